"""fp64 references, an elementwise error bound, input generators and mutated references for the two encoder attention kernels of
csrc/attention.hip (window_attention_kernel, global_attention_kernel).  A plain module: no fixtures, no kernel calls.  Everything is
torch and follows the device of its operands, so the GPU tests compute the references in fp64 on the device, one (image, head) at a time.

The operation (SAM's attention with decomposed relative position bias) on 16-bit q, k, v [B, heads, 4096, hs] - hs the STORED head_dim,
of which the first ``head_dim`` channels are real and the rest zero padding:

    s[i, j] = scale * q_i . k_j + q_i . rel_h[ih - jh + S - 1] + q_i . rel_w[iw - jw + S - 1],     out_i = softmax_j(s[i, :]) @ v

global: S = 64, all 4096 tokens of an image.  window: S = 14, the 64 x 64 grid is padded to 70 x 70 and cut into 5 x 5 windows; a padding
token carries the projection bias alone (the layer input is zero there) rounded to the 16-bit type, it is a key like any other, and its
own output is dropped.

The bound (``_bound``) comes from the kernels' rounding points.  Both kernels form the scores and exp() in fp32, round the un-normalised
probabilities p to the 16-bit type before P V, sum l from the UNROUNDED p, accumulate P V in fp32 and round o / l once to the 16-bit type.
With P the fp64 softmax and u the unit roundoff of the type (2^-8 bf16, 2^-11 fp16):

    |got - ref|[i, c] <= (2 u + 2 * 2^-20 * (1 + max_j |s[i, j]|)) * (P @ |v|)[i, c]            (+ 2^-25 * sum_j |v[j, c]| in fp16)

u (P @ |v|) for the rounded probabilities, u |ref| <= u (P @ |v|) for the output; the second term of the bracket covers the fp32 score
(relative 2^-24 of a magnitude up to max |s|, which exp() turns into a relative error of p) and v_exp_f32, and is negligible against u while
|s| stays below about 60 - the generators keep it there.  The fp16 extra covers probabilities below fp16's normal range 2^-14, whose
absolute rounding error is up to 2^-25 of the row's largest probability.

MUTATIONS names the defects these kernels are prone to, written as variants of the references; tests/test_attention_ref_host.py proves
that each is at least 4 bounds from the truth on the generator meant for it, so a kernel within one bound of the truth cannot have it."""
import math

import torch

TOK = 4096
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

MUTATIONS = ("rel_h_plus1", "rel_w_plus1", "rel_swap_hw", "rel_sign", "drop_last32", "drop_192", "swap_v_rows", "pad_zero",
             "pad_masked", "swap_heads", "image1_from_image0", "scale_96")
_ONE_HEAD = ("rel_h_plus1", "rel_w_plus1", "rel_swap_hw", "rel_sign", "drop_last32", "drop_192", "swap_v_rows", "pad_zero", "pad_masked")
SWAP_V = (1000, 1001)                 # global: the two keys whose value rows "swap_v_rows" exchanges; window: local tokens 100 and 101


def round16(t, dtype):
    return t.to(dtype).double()


def _bound(s, p, v, dtype):
    """s, p [..., Q, K] fp64 scores / softmax, v [..., K, C] fp64 -> the elementwise bound [..., Q, C] of the module docstring."""
    smax = s.abs().amax(dim=-1, keepdim=True)
    b = (2.0 * U[dtype] + 2.0 * 2.0 ** -20 * (1.0 + smax)) * (p @ v.abs())
    if dtype == torch.float16:
        b = b + 2.0 ** -25 * v.abs().sum(dim=-2, keepdim=True)
    return b


def _rel_terms(qg, rh, rw, S, mutation):
    """qg [..., S, S, C] queries on their grid, tables [2 S - 1, C] -> (th [..., S, S, kh], tw [..., S, S, kw])."""
    idx = torch.arange(S, device=qg.device)
    d = idx[:, None] - idx[None, :]                                               # [query coordinate, key coordinate]
    if mutation == "rel_sign":
        d = -d
    d = d + S - 1
    dh = (d + 1) % (2 * S - 1) if mutation == "rel_h_plus1" else d
    dw = (d + 1) % (2 * S - 1) if mutation == "rel_w_plus1" else d
    if mutation == "rel_swap_hw":
        rh, rw = rw, rh
    th = torch.einsum("...hwc,hkc->...hwk", qg, rh[dh])
    tw = torch.einsum("...hwc,wkc->...hwk", qg, rw[dw])
    return th, tw


def global_attention_one(q, k, v, rel_h, rel_w, scale, dtype, mutation=None):
    """One (image, head): fp64 q, k, v [4096, C] and tables [127, C] (the values of 16-bit operands) -> (ref, bound), each [4096, C]."""
    assert mutation is None or mutation in _ONE_HEAD, mutation
    C = q.shape[-1]
    th, tw = _rel_terms(q.reshape(64, 64, C), rel_h, rel_w, 64, mutation)
    s = ((scale * q @ k.t()).reshape(64, 64, 64, 64) + th[:, :, :, None] + tw[:, :, None, :]).reshape(TOK, TOK)
    del th, tw
    if mutation == "drop_last32":
        s[:, TOK - 32:] = -math.inf
    if mutation == "swap_v_rows":
        v = v.clone()
        v[list(SWAP_V)] = v[list(SWAP_V[::-1])]
    p = torch.softmax(s, dim=-1)
    s.nan_to_num_(neginf=0.0)
    return p @ v, _bound(s, p, v, dtype)


def _windows(t, pad_row):
    """[4096, C] tokens of the image, [C] value of a padding token -> [25, 196, C] tokens of the 5 x 5 windows of the 70 x 70 grid."""
    C = t.shape[-1]
    g = pad_row.expand(70, 70, C).clone()
    g[:64, :64] = t.reshape(64, 64, C)
    return g.reshape(5, 14, 5, 14, C).permute(0, 2, 1, 3, 4).reshape(25, 196, C)


def _unwindow(o):
    """[25, 196, C] -> [4096, C]: the real tokens."""
    C = o.shape[-1]
    return o.reshape(5, 5, 14, 14, C).permute(0, 2, 1, 3, 4).reshape(70, 70, C)[:64, :64].reshape(TOK, C)


def window_attention_one(q, k, v, rel_h, rel_w, bq, bk, bv, scale, dtype, mutation=None):
    """One (image, head): fp64 q, k, v [4096, C], tables [27, C], fp64 bias rows [C] ALREADY rounded to the 16-bit type ->
    (ref, bound), each [4096, C]."""
    assert mutation is None or mutation in _ONE_HEAD, mutation
    C = q.shape[-1]
    if mutation == "pad_zero":
        bk, bv = torch.zeros_like(bk), torch.zeros_like(bv)
    qs, ks, vs = _windows(q, bq), _windows(k, bk), _windows(v, bv)
    th, tw = _rel_terms(qs.reshape(25, 14, 14, C), rel_h, rel_w, 14, mutation)
    s = ((scale * qs @ ks.transpose(1, 2)).reshape(25, 14, 14, 14, 14) + th[..., :, None] + tw[..., None, :]).reshape(25, 196, 196)
    if mutation == "drop_192":
        s[:, :, 192:] = -math.inf
    if mutation == "pad_masked":
        real = _windows(torch.ones(TOK, 1, dtype=q.dtype, device=q.device), torch.zeros(1, dtype=q.dtype, device=q.device))[:, :, 0] > 0
        s = s.masked_fill(~real[:, None, :], -math.inf)
    if mutation == "swap_v_rows":
        vs = vs.clone()
        vs[:, [100, 101]] = vs[:, [101, 100]]
    p = torch.softmax(s, dim=-1)
    s.nan_to_num_(neginf=0.0)
    return _unwindow(p @ vs), _unwindow(_bound(s, p, vs, dtype))


def attention_ref(kind, inp, mutation=None, pairs=None):
    """``inp``: a dict of a generator below (q, k, v [B, heads, 4096, hs] 16 bit, rel_h, rel_w [2 S - 1, hs], qkv_bias fp32
    [3 heads hs] for windows, scale, head_dim).  -> (ref, bound) fp64 [B * 4096, heads * hs] in the kernels' output layout, computed one
    (image, head) at a time on the operands' device from the first head_dim channels; padded channels: ref 0, bound 0.
    ``pairs``: only these (image, head) are computed (the rest of ref / bound stays 0)."""
    assert kind in ("window", "global") and (mutation is None or mutation in MUTATIONS), (kind, mutation)
    q, k, v = inp["q"], inp["k"], inp["v"]
    B, heads, _, hs = q.shape
    hd, dtype, scale = inp["head_dim"], q.dtype, inp["scale"]
    if mutation == "scale_96":
        assert hs == 96 and hd == 80
        scale = 96 ** -0.5
    rh, rw = inp["rel_h"].double()[:, :hd], inp["rel_w"].double()[:, :hd]
    ref = torch.zeros(B, TOK, heads, hs, dtype=torch.float64, device=q.device)
    bound = torch.zeros_like(ref)
    for b in range(B):
        for h in range(heads):
            if pairs is not None and (b, h) not in pairs:
                continue
            sb = 0 if mutation == "image1_from_image0" else b                     # source image / head of this output slot
            sh = (h + 1) % heads if mutation == "swap_heads" else h
            one = mutation if mutation in _ONE_HEAD else None
            qd, kd, vd = (t[sb, sh, :, :hd].double() for t in (q, k, v))
            if kind == "global":
                r, bd = global_attention_one(qd, kd, vd, rh, rw, scale, dtype, one)
            else:
                bias = inp["qkv_bias"].reshape(3, heads, hs)[:, sh, :hd]
                bq, bk, bv = (round16(bias[i], dtype) for i in range(3))
                r, bd = window_attention_one(qd, kd, vd, rh, rw, bq, bk, bv, scale, dtype, one)
            ref[b, :, h, :hd], bound[b, :, h, :hd] = r, bd
    return ref.reshape(B * TOK, heads * hs), bound.reshape(B * TOK, heads * hs)


# --------------------------------------------------------------------------------------------------------------------- generators
GENERATORS = {"window": ("peaked", "diffuse", "needle", "rel_only", "padding", "padding_aligned"),
              "global": ("peaked", "diffuse", "needle", "rel_only")}


def _window_real_tokens():
    """Per window: the image token indices of its real (non-padding) tokens, in window order."""
    y = torch.arange(70)
    tok = (y[:, None] * 64 + y[None, :]).masked_fill((y[:, None] >= 64) | (y[None, :] >= 64), -1)
    w = tok.reshape(5, 14, 5, 14).permute(0, 2, 1, 3).reshape(25, 196)
    return [row[row >= 0] for row in w]


def make_inputs(kind, name, dtype, hs, B=1, heads=1, seed=0):
    """Seeded operands of one kernel call, on the CPU, independent data per (image, head).  hs 64: head_dim 64; hs 96: head_dim 80,
    channels 80.. of q, k, v, the tables and the bias zero; scale = head_dim ** -0.5.

    peaked           q x 3: a few keys carry a row, the running maximum of the global kernel still moves in late key tiles
    diffuse          q x 0.25: near-uniform rows, the running maximum rarely moves after the first tiles
    needle           k = +-1 codes, q_i = 4 k_pi(i) for a random permutation pi (inside each window's real tokens for windows), zero
                     tables and q / k bias: every query puts >= 0.9999 of its weight on key pi(i), so the output is v[pi(i)] within the
                     bound and any wrong key -> value mapping (LDS swizzle, transposing read, tile order, t0 / t1 pairing) is a wrong row
    rel_only         k = 0 (and zero k bias): the scores are the two bias terms alone, tables scaled for a peaked softmax; global: the
                     queries at the four image corners are aligned with table rows 0 and 126, which then carry their rows' weight
    padding          windows: qkv_bias of std 1, so the bias-only tokens of the edge windows matter as keys and values
    padding_aligned  the same with q = b_k + noise: in the edge windows the bias-only keys take nearly all the weight and the output
                     there is close to round16(b_v)"""
    assert name in GENERATORS[kind] and hs in (64, 96) and dtype in U, (kind, name, hs, dtype)
    hd = 64 if hs == 64 else 80
    S = 14 if kind == "window" else 64
    g = torch.Generator().manual_seed(1000 * seed + 17 * GENERATORS["window"].index(name) + (kind == "global") + 2 * (hs == 96))

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    q, k, v = rn(B, heads, TOK, hd), rn(B, heads, TOK, hd), rn(B, heads, TOK, hd)
    rel_h, rel_w = rn(2 * S - 1, hd) * 0.1, rn(2 * S - 1, hd) * 0.1
    bias = rn(3, heads, hd) * 0.3
    if name == "peaked":
        q = q * 3.0
    elif name == "diffuse":
        q = q * 0.25
    elif name == "needle":
        k = torch.where(k > 0, 1.0, -1.0)
        src = torch.empty(B, heads, TOK, dtype=torch.long)
        for b in range(B):
            for h in range(heads):
                if kind == "global":
                    src[b, h] = torch.randperm(TOK, generator=g)
                else:
                    for toks in _window_real_tokens():
                        src[b, h, toks] = toks[torch.randperm(len(toks), generator=g)]
        q = 4.0 * torch.gather(k, 2, src[..., None].expand(-1, -1, -1, hd))
        rel_h, rel_w = torch.zeros_like(rel_h), torch.zeros_like(rel_w)
        bias[:2] = 0.0
    elif name == "rel_only":
        k = torch.zeros_like(k)
        bias[1] = 0.0
        rel_h, rel_w = rn(2 * S - 1, hd) * 0.5, rn(2 * S - 1, hd) * 0.5
        if kind == "global":
            for tok, ih, iw in ((0, 0, 0), (63, 0, 126), (63 * 64, 126, 0), (TOK - 1, 126, 126)):
                q[:, :, tok] = 0.6 * (rel_h[ih] + rel_w[iw])
    elif name == "padding":
        bias = rn(3, heads, hd)
    elif name == "padding_aligned":
        bias = rn(3, heads, hd)
        q = bias[1].to(dtype).float()[None, :, None, :] + 0.5 * q
        rel_h, rel_w = rel_h * 0.5, rel_w * 0.5
    pad = (0, hs - hd)
    out = {name_: torch.nn.functional.pad(t, pad).to(dtype).contiguous() for name_, t in (("q", q), ("k", k), ("v", v), ("rel_h", rel_h), ("rel_w", rel_w))}
    out.update(scale=hd ** -0.5, head_dim=hd)
    if kind == "window":
        out["qkv_bias"] = torch.nn.functional.pad(bias, pad).reshape(-1).float().contiguous()
    return out
