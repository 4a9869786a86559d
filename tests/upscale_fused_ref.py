"""fp64 reference, elementwise error bound, rounded restatement, input generators and mutated references for up_fused_kernel
(csrc/upfused.hip: msam_upscale_fused / _layout / _out / _range).  A plain module: no fixtures, no kernel calls.  Everything is torch and
follows the device of its operands; the reference works in chunks of prompts.

THE OPERATION, on the VALUES of the 16-bit operands, in the reference model's formulation (so the transposed, fused form is under test).
A prompt's stream is a 64 x 64 grid of tokens t = 64 ty + tx with 256 channels; s = 2 dy + dx and r = 2 dy2 + dx2 are the sub-pixels of the
two transposed convolutions:

  u[t, s, c]    = sum_k w1[64 s + c, k] keys[t, k] + b1[64 s + c]                    ConvT(256 -> 64, 2 x 2, stride 2), c < 64
  x1[t, s, c]   = (u - mu) / sqrt(var + eps) ln_w[c] + ln_b[c]                       LayerNorm2d over the 64 c of a (t, s)
  y[t, s, r, d] = sum_c w2[32 r + d, c] G(x1[t, s, c]) + b2[d]                       ConvT(64 -> 32, 2 x 2, stride 2), d < 32;  G = erf-GELU
  out[m, 4 ty + 2 dy + dy2, 4 tx + 2 dx + dx2] = sum_d hyper[mask0 + m, d] G(y[t, s, r, d])                            m < nmask

``ref`` takes the weight layout of the entry point (w1 [256, 256], b1 [256], w2 [128, 64], hyper [P, 4, ld]).  With ``centred`` weights it
is the function of the weights HANDED OVER: their fp16 rounding is the caller's, not a kernel error - but the mean the rounded weights
still have is LayerNorm2d's to remove, and a kernel that does not compute it (CEN) owes it to the bound below.

THE BOUND.  u = 2^-8 (bf16) / 2^-11 (fp16) is the unit roundoff of the decoder's 16-bit type, SUB = 2^-25 the absolute rounding error below
fp16's normal range (0 for bf16), UH = 2^-11 and SUBH = 2^-25 those of fp16 (G2, the hyper pair and the fp16 output are fp16 in both
builds), F = 2^-24 the unit roundoff of fp32.  Term by term from the kernel's rounding points:

  * stage 1, an fp32 MFMA chain of 8 k-steps of 32 products on the bias as initial value, each step summed in an unspecified order: a
    product passes <= 32 roundings in its own step and one per later step, 40 F (|w1| |keys| + |b1|) =: E elementwise.
  * LayerNorm2d, carried through WITHOUT linearising.  With mu, dev = u - mu, sig = sqrt(var + eps) of the reference and the kernel's
    |mu' - mu| <= Ebar, |dev' - dev| <= E + Ebar, |sig' - sig| <= E2 (centring is a projection, x -> sqrt(x^2 + eps) is 1-Lipschitz):
        |z' - z| <= (E + Ebar) / (sig - E2) + |dev| E2 / (sig (sig - E2)),    z = dev / sig.
    Sums of 64 fp32 values (16 in a lane, two cross-lane steps) carry <= 20 F of the sum of magnitudes, sums of squares (products
    rounded as well) <= 40 F.  m1 = mean(|u| + E), m2 = mean((|u| + E)^2).
      one pass   mean' within 20 F m1 of mean(u'); var' = fl(fl(ss / 64) - fl(mean'^2)): 40 F m2 (the sum of squares) + 38 F m2 (the
                 squared mean: 2 |mean| 20 F m1 + its rounding, |mean| m1 <= m2) + 2 F m2 (the subtraction, + eps) = 80 F m2 =: dvar.  THIS
                 is the E[u^2] / var loss: dvar is relative to E[u^2], not to var.  Ebar = mean(E) + 20 F m1, E2 = rms(E) + ds(dvar),
                 where |sqrt(a + d) - sqrt(a)| <= ds(d) := min(sqrt(d), d / sqrt(a)) and a >= (sig - rms(E))^2.  (The clamp
                 max(var', 0) only moves var' towards the true value, which is >= 0.)
      two pass   the same mean; the variance is the mean of squares of the CENTRED values: dvar = 40 F mean((|dev| + E + Ebar)^2), and a
                 centre off by 20 F m1 moves the rms by at most that: E2 = rms(E) + 20 F m1 + ds(dvar).
      CEN        no mean at all: mu' = 0, so Ebar = |mu| (the mean the handed-over weights give - known exactly from the reference),
                 dev' = u', sig' = sqrt(mean(u'^2) + eps): E2 = rms(E) + |mu| + ds(40 F m2).
    rsqrt (1 ulp), the two products and the multiply-add of the affine step: 8 F (|u| + |mu| + E) |ln_w| / (sig - E2) + 2 F |ln_b|.
    Together e_x1, the error of the first GELU's argument.
  * a GELU, given an argument error e_x.  erf-GELU's slope is at most 1.13 (GELU_SLOPE).  Both kernels evaluate
        Fm(x) = max(x, 0) - |x| 2^q(|x|),  q a cubic (gelu_erf2 of common.h),
    whose distance from erf-GELU is a property of the formula: A_FORMULA = sup |Fm - G|, measured below in fp64 over all finite fp16 inputs and
    a dense grid (5.5e-5).
      packed fp32 (gelu_erf2)   |x| = 2 max(x, 0) - x is exact; three multiply-adds give q with <= 3 F Q(|x|) (Q = the cubic's magnitude: all its
                 terms have one sign), v_exp_f32 is 1 ulp: relative error of the exponential <= F (3 ln2 Q + 2), times |x| 2^-Q <= K32 F (K32 =
                 the sup of |x| 2^-Q (3 ln2 Q + 2), measured below); the last multiply-add F |g|.  Then ONE rounding to the 16-bit type.
                     1.13 e_x + A_FORMULA + (K32 + 2) F + F |g|,  then  u |g'| + SUB.
      packed fp16 (gelu_pk_h2)  a RUNNING error analysis of its nine fp16 operations (convert, max, multiply-add for |x|, three for the
                 cubic, two exponentials, the last multiply-add), each result rounded once (UH, SUBH), the cubic's constants being the
                 fp16 roundings c' of the formula's c:
                     et = e_x + UH (|x| + e_x) + SUBH                                   the conversion; max and |x| are exact
                     e1 = |c3| et + |c3' - c3| (t + et) + |c2' - c2|, + UH (|q1| + e1) + SUBH       q1 = c3 t + c2
                     e2 = e1 (t + et) + |q1| et + |c1' - c1|,         + UH (|q2| + e2) + SUBH       q2 = q1 t + c1
                     e3 = e2 (t + et) + |q2| et + |c0' - c0|,         + UH (|q3| + e3) + SUBH       q3 = q2 t + c0
                     ee = 2^q3 (2^e3 - 1) + 2 UH 2^q3 2^e3 + 2 SUBH                     v_exp_f16 at 1 ulp (see below)
                     eg = et + et (2^q3 + ee) + t ee,                 + UH (|Fm(x)| + eg) + SUBH
                 and A_FORMULA on top.  Its result IS the 16-bit operand: no further rounding.  (tests/test_upscale_fused_ref_host.py runs
                 the emulated nine operations over all 65536 fp16 inputs against this analysis.)
    v_exp_f16's accuracy: the ISA documentation is not at hand; 1 ulp is ASSUMED (the figure AMD's ISA guides give for the fp32
    transcendentals).  The restatement rounds the exponential correctly (1/2 ulp); the mean criterion's margin covers the difference.
  * stage 2, an fp32 chain of 2 k-steps on the bias: e_y = |w2| e_g1 + 34 F (|w2| (|G1| + e_g1) + |b2|).  The second GELU as above, its output
    rounded to fp16 in BOTH builds (it is stage 3's fp16 operand): e_g2.
  * stage 3: the hyper weights enter as an fp16 pair hi = fp16(h), lo = fp16(h - hi) (the difference is exact in fp32):
    |h - hi - lo| <= 2^-22 |h| + SUBH =: e_h, the subnormal floor being lo's absolute rounding error.  Two MFMAs of 32 products: 34 F.
        e_out = |h| e_g2 + (e_h + 34 F |h|) (|G2| + e_g2)
  * the optional fp16 rounding of the output: UH (|out| + e_out) + SUBH.

DOMAIN: |hyper| and G2 stay inside fp16's range (65504) - the kernel packs both to fp16 and is not asked to survive more - and
sig - E2 > 0 (else the bound is infinite).  The generators keep to it; the host test checks that they do.

``restate`` redoes the arithmetic in fp64 with a rounding at exactly those points, for both GELU forms: it must lie within one bound of
the reference, which keeps the bound honest from below, and its mean error per (prompt, mask) plane is what a correct kernel's mean error
is compared with (the device test: mean |got - ref| <= 1.5 mean |restate - ref|).  MUTATIONS names the defects this kernel is prone to as
variants of the reference."""
import math

import torch

T, C, C1, C2 = 4096, 256, 64, 32
TK = 16                                                   # tokens of a tile
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
UH, SUBH = 2.0 ** -11, 2.0 ** -25
F32 = 2.0 ** -24
LN_EPS = 1e-6
GELU_SLOPE = 1.13
MEAN_MARGIN = 1.5

ROUTE_LN = ("one_pass", "two_pass", "cen")
GENERATORS = ("diffuse", "wide", "flat", "large_mean", "hyper_pair")
MUTATIONS = ("last_tile_not_stored", "last_tile_next_base", "first_tile_stale_hyper", "tile_repeated_at_clamp", "split_rows_crossed",
             "subpixels_crossed", "mask0_ignored", "mask_rows_crossed", "hyper_ld_128", "hyper_channels_32", "no_b1", "no_b2", "no_ln_b",
             "no_eps", "eps_slip", "ln_wrong_64", "blocked_as_row_major", "tanh_gelu", "hyper_lo_dropped", "out16_truncated")


def f32(x):
    """The value of a float argument of the C entry point."""
    return float(torch.tensor(x, dtype=torch.float32))


# the cubic of gelu_erf2 (common.h): 2^q(t), q = ((c3 t + c2) t + c1) t + c0
CUBIC = tuple(f32(c) for c in (-0.0248758, -0.49884797, -1.12922424, -1.00353579))               # c3, c2, c1, c0
CUBIC_H = tuple(float(torch.tensor(c, dtype=torch.float16)) for c in CUBIC)                      # what gelu_pk_h2 multiplies by


def route(ln="cen", gelu16=True, out16=False):
    """An instantiation of the kernel: LayerNorm statistics ("one_pass", "two_pass", "cen"), packed-fp16 or packed-fp32 GELUs, fp16 output."""
    assert ln in ROUTE_LN
    return {"ln": ln, "gelu16": bool(gelu16), "out16": bool(out16)}


def key_splits(P, cus):
    """(KS, grid) of msam_upscale_fused_range: the smallest power of two with P * KS >= 2 * cus, at most 16; min(P * KS, 2 * cus)
    workgroups.  A work item is one of the KS key splits (4096 / KS tokens) of a prompt; workgroup b runs items b, b + grid, ..."""
    ks = 1
    while P * ks < 2 * cus and ks < 16:
        ks *= 2
    return ks, min(P * ks, 2 * cus)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _cubic(t, c):
    q1 = c[0] * t + c[1]
    q2 = q1 * t + c[2]
    return q1, q2, q2 * t + c[3]


def gelu_formula(x):
    """Fm of the docstring in fp64."""
    r = x.clamp(min=0.0)
    t = 2.0 * r - x
    return r - t * torch.exp2(_cubic(t, CUBIC)[2])


def rh(x):
    return x.to(torch.float16).double()


def round16(x, dtype):
    return x.to(dtype).double()


def gelu_pk16(x):
    """gelu_pk_h2 step by step: every operation in fp64 followed by ONE rounding to fp16 (the products of fp16 values and their sums with a
    third are exact in fp64 wherever the result's rounding can tell), the exponential correctly rounded."""
    x = rh(x)
    r = x.clamp(min=0.0)
    t = rh(2.0 * r - x)
    q = rh(t * CUBIC_H[0] + CUBIC_H[1])
    q = rh(q * t + CUBIC_H[2])
    q = rh(q * t + CUBIC_H[3])
    return rh(r - t * rh(torch.exp2(q)))


def _all_fp16(dev="cpu"):
    h = torch.arange(65536, dtype=torch.int32, device=dev).to(torch.int16).view(torch.float16).double()
    return h[torch.isfinite(h)]


def _measure():
    x = torch.cat([_all_fp16(), torch.linspace(-16.0, 16.0, (1 << 20) + 1, dtype=torch.float64)])
    a = float((gelu_formula(x) - gelu_erf(x)).abs().max())
    t = torch.linspace(0.0, 64.0, (1 << 20) + 1, dtype=torch.float64)
    Q = _cubic(t, tuple(abs(c) for c in CUBIC))[2]
    return a, float((t * torch.exp2(-Q) * (3.0 * math.log(2.0) * Q + 2.0)).max())


A_FORMULA, K32 = _measure()


def gelu_err(x, ex, gelu16, u_out, sub_out):
    """|the kernel's GELU output - G(x)| for a kernel argument within ``ex`` of ``x``: the GELU paragraph of the docstring."""
    if not gelu16:
        g = gelu_erf(x).abs()
        core = GELU_SLOPE * ex + A_FORMULA + (K32 + 2.0) * F32 + F32 * g
        return core + u_out * (g + core) + sub_out
    c, ch = CUBIC, CUBIC_H
    t = x.abs()
    q1, q2, q3 = _cubic(t, c)
    et = ex + UH * (t + ex) + SUBH
    tt = t + et
    e1 = abs(c[0]) * et + abs(ch[0] - c[0]) * tt + abs(ch[1] - c[1])
    e1 = e1 + UH * (q1.abs() + e1) + SUBH
    e2 = e1 * tt + q1.abs() * et + abs(ch[2] - c[2])
    e2 = e2 + UH * (q2.abs() + e2) + SUBH
    e3 = e2 * tt + q2.abs() * et + abs(ch[3] - c[3])
    e3 = e3 + UH * (q3.abs() + e3) + SUBH
    e = torch.exp2(q3)
    grow = torch.exp2(e3.clamp(max=64.0))
    ee = e * (grow - 1.0) + 2.0 * UH * e * grow + 2.0 * SUBH
    eg = et + et * (e + ee) + t * ee
    eg = eg + UH * (gelu_formula(x).abs() + eg) + SUBH
    return eg + A_FORMULA


# ------------------------------------------------------------------------------------------------------------------- the operation
def to_blocked(x):
    """[..., 4096, W] row-major -> the blocked stream layout of csrc/decfold_tok.hip ([16-token tile][k-step of 32 channels][lane group]
    [token][8 channels]), flattened back to [..., 4096, W]."""
    W = x.shape[-1]
    lead = x.shape[:-2]
    n = len(lead)
    y = x.reshape(*lead, 256, 16, W // 32, 4, 8).permute(*range(n), n, n + 2, n + 3, n + 1, n + 4)
    return y.reshape(*lead, T, W).contiguous()


def pixels(o, crossed=False):
    """[n, m, T, 4 (s), 4 (r)] -> [n, m, 256, 256]: pixel (4 ty + 2 dy + dy2, 4 tx + 2 dx + dx2)."""
    n, m = o.shape[:2]
    o = o.reshape(n, m, 64, 64, 2, 2, 2, 2)                                               # ty, tx, dy, dx, dy2, dx2
    o = o.permute(0, 1, 2, 6, 4, 3, 7, 5) if crossed else o.permute(0, 1, 2, 4, 6, 3, 5, 7)
    return o.reshape(n, m, 256, 256)


def unpixels(o):
    """Inverse of ``pixels``."""
    n, m = o.shape[:2]
    return o.reshape(n, m, 64, 2, 2, 64, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(n, m, T, 4, 4)


def _hyper_rows(inp, lo, hi, mutation=None):
    """fp64 [n, nmask, 32]"""
    h, m0, nm = inp["hyper"], inp["mask0"], inp["nmask"]
    if mutation == "mask0_ignored":
        m0 = 0
    if mutation == "hyper_ld_128":                       # row (4 p + mask) read 128 floats apart in the buffer (indices taken modulo its size)
        flat = h.reshape(-1)
        p = torch.arange(lo, hi, device=h.device)[:, None, None]
        idx = ((4 * p + m0 + torch.arange(nm, device=h.device)[None, :, None]) * 128 + torch.arange(C2, device=h.device)) % flat.numel()
        return flat[idx].double()
    c0 = C2 if mutation == "hyper_channels_32" else 0
    return h[lo:hi, m0:m0 + nm, c0:c0 + C2].double()


def _first_stages(inp, lo, hi, mutation=None):
    """Everything up to G2 in fp64 for prompts [lo, hi): a dict of u [n, T, 4, 64], mu, dev, sig, x1, g1, y [n, T, 4, 4, 32], g2."""
    X = inp["keys"][lo:hi].double()
    if mutation == "blocked_as_row_major":
        X = to_blocked(X)
    w1, b1 = inp["w1"].double(), inp["b1"].double()
    w2, b2 = inp["w2"].double(), inp["b2"].double()
    lw, lb = inp["ln_w"].double(), inp["ln_b"].double()
    eps = {"no_eps": 0.0, "eps_slip": 10.0}.get(mutation, 1.0) * f32(inp["eps"])             # eps_slip: 1e-5 for 1e-6, say
    if mutation == "no_b1":
        b1 = torch.zeros_like(b1)
    if mutation == "no_b2":
        b2 = torch.zeros_like(b2)
    if mutation == "no_ln_b":
        lb = torch.zeros_like(lb)
    gelu = gelu_tanh if mutation == "tanh_gelu" else gelu_erf
    n = X.shape[0]
    u = (X @ w1.t() + b1).reshape(n, T, 4, C1)
    if mutation == "ln_wrong_64":                        # statistics over 16 channels of each of the four sub-pixels
        grp = u.reshape(n, T, 4, 4, 16).transpose(2, 3).reshape(n, T, 4, C1)
        mu = grp.mean(dim=-1, keepdim=True)
        var = ((grp - mu) ** 2).mean(dim=-1, keepdim=True)
    else:
        mu = u.mean(dim=-1, keepdim=True)
        var = ((u - mu) ** 2).mean(dim=-1, keepdim=True)
    dev = u - mu
    sig = torch.sqrt(var + eps)
    x1 = dev / sig * lw + lb
    g1 = gelu(x1)
    y = (g1 @ w2.t()).reshape(n, T, 4, 4, C2) + b2
    return {"X": X, "u": u, "mu": mu, "dev": dev, "sig": sig, "x1": x1, "g1": g1, "y": y, "g2": gelu(y)}


def _project(h, g2):
    """[n, m, 32] x [n, T, 4, 4, 32] -> [n, m, T, 4, 4]"""
    return torch.einsum("nmd,ntsrd->nmtsr", h, g2)


def _bound(inp, lo, hi, st, h, out, rt, with_g2=False):
    """The bound of the module docstring for prompts [lo, hi); ``with_g2``: (bound, e_g2) instead."""
    dtype = inp["keys"].dtype
    u16, sub = U[dtype], SUB[dtype]
    F = F32
    n = st["u"].shape[0]
    w1, b1 = inp["w1"].double(), inp["b1"].double()
    w2, b2 = inp["w2"].double(), inp["b2"].double()
    lw, lb = inp["ln_w"].double(), inp["ln_b"].double()
    u, mu, dev, sig = st["u"], st["mu"], st["dev"], st["sig"]
    E = 40 * F * (st["X"].abs() @ w1.abs().t() + b1.abs()).reshape(n, T, 4, C1)
    rmsE = torch.sqrt((E * E).mean(dim=-1, keepdim=True))
    m1 = (u.abs() + E).mean(dim=-1, keepdim=True)
    m2 = ((u.abs() + E) ** 2).mean(dim=-1, keepdim=True)
    if rt["ln"] == "cen":
        Ebar, dvar, E2 = mu.abs(), 40 * F * m2, rmsE + mu.abs()
    elif rt["ln"] == "two_pass":
        Ebar = E.mean(dim=-1, keepdim=True) + 20 * F * m1
        dvar = 40 * F * ((dev.abs() + E + Ebar) ** 2).mean(dim=-1, keepdim=True)
        E2 = rmsE + 20 * F * m1
    else:
        Ebar, dvar, E2 = E.mean(dim=-1, keepdim=True) + 20 * F * m1, 80 * F * m2, rmsE
    a = (sig - E2).clamp(min=0.0)
    E2 = E2 + torch.minimum(torch.sqrt(dvar), dvar / a)
    den = sig - E2
    ex1 = lw.abs() * ((E + Ebar) / den + dev.abs() * E2 / (sig * den)) + 8 * F * (u.abs() + mu.abs() + E) * lw.abs() / den + 2 * F * lb.abs()
    ex1 = torch.where(den > 0, ex1, torch.full_like(ex1, float("inf")))                  # (outside the domain: the bound is infinite)
    g16 = rt["gelu16"]
    eg1 = gelu_err(st["x1"], ex1, g16, UH if g16 else u16, SUBH if g16 else sub)
    g1a = st["g1"].abs() + eg1
    ey = (eg1 @ w2.abs().t() + 34 * F * (g1a @ w2.abs().t())).reshape(n, T, 4, 4, C2) + 34 * F * b2.abs()
    eg2 = gelu_err(st["y"], ey, g16, UH, SUBH)
    eh = 2.0 ** -22 * h.abs() + SUBH
    eo = _project(h.abs(), eg2) + _project(eh + 34 * F * h.abs(), st["g2"].abs() + eg2)
    if rt["out16"]:
        eo = eo + UH * (out.abs() + eo) + SUBH
    return (eo, eg2) if with_g2 else eo


def ref_chunks(inp, rt, chunk=8):
    """Yields (lo, hi, ref, bound), fp64 [hi - lo, nmask, 256, 256], chunk by chunk of prompts."""
    P = inp["keys"].shape[0]
    for lo in range(0, P, chunk):
        hi = min(lo + chunk, P)
        st = _first_stages(inp, lo, hi)
        h = _hyper_rows(inp, lo, hi)
        out = _project(h, st["g2"])
        yield lo, hi, pixels(out), pixels(_bound(inp, lo, hi, st, h, out, rt))


def ref(inp, rt=None, chunk=8):
    """``inp``: a dict of ``make`` -> (ref, bound of route ``rt``) fp64 [P, nmask, 256, 256]; without a route (ref, None)."""
    if rt is None:
        P = inp["keys"].shape[0]
        return torch.cat([pixels(_project(_hyper_rows(inp, lo, min(lo + chunk, P)), _first_stages(inp, lo, min(lo + chunk, P))["g2"]))
                          for lo in range(0, P, chunk)]), None
    parts = list(ref_chunks(inp, rt, chunk))
    return torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])


def diff_bound_chunks(inp, hyper_d, rt, chunk=8):
    """The differential check: yields (lo, hi, expected out(a + d) - out(a) = d . G2, its bound): the bound's last stage with d = hyper_d - hyper
    in place of hyper, plus the fp32 accumulation term of a in both launches."""
    P = inp["keys"].shape[0]
    for lo in range(0, P, chunk):
        hi = min(lo + chunk, P)
        st = _first_stages(inp, lo, hi)
        a = _hyper_rows(inp, lo, hi)
        d = _hyper_rows(dict(inp, hyper=hyper_d), lo, hi) - a
        # the two launches compute the SAME G2' (per-token arithmetic does not depend on the hyper weights), so G2's own error enters with |d| only
        full, eg2 = _bound(inp, lo, hi, st, d, _project(d, st["g2"]), dict(rt, out16=False), with_g2=True)
        acc = 2 * _project(34 * F32 * (a.abs() + d.abs()), st["g2"].abs() + eg2)         # the two MFMAs' roundings, in either launch
        yield lo, hi, pixels(_project(d, st["g2"])), pixels(full + acc)


def restate(inp, rt, chunk=8, mutation=None):
    """The kernel's arithmetic in fp64 with a rounding at exactly its rounding points (docstring); [P, nmask, 256, 256] fp64.
    ``mutation``: "hyper_lo_dropped", "out16_truncated" (the two defects that are defects of the ROUNDED arithmetic) or "tanh_gelu" (the tanh
    approximation, rounded once, in place of either GELU form: what the mean criterion is shown to catch)."""
    dtype = inp["keys"].dtype
    P = inp["keys"].shape[0]
    w1, b1 = inp["w1"].double(), inp["b1"].double()
    w2, b2 = inp["w2"].double(), inp["b2"].double()
    lw, lb = inp["ln_w"].double(), inp["ln_b"].double()
    eps = f32(inp["eps"])
    outs = []
    for lo in range(0, P, chunk):
        X = inp["keys"][lo:lo + chunk].double()
        n = X.shape[0]
        u = (X @ w1.t() + b1).reshape(n, T, 4, C1)
        if rt["ln"] == "cen":
            dev, var = u, (u * u).mean(dim=-1, keepdim=True)
        else:
            mean = u.mean(dim=-1, keepdim=True)
            dev = u - mean
            if rt["ln"] == "two_pass":
                var = (dev * dev).mean(dim=-1, keepdim=True)
            else:
                var = ((u * u).mean(dim=-1, keepdim=True) - mean * mean).clamp(min=0.0)
        x1 = dev * torch.rsqrt(var + eps) * lw + lb
        d1 = torch.float16 if rt["gelu16"] else dtype
        if mutation == "tanh_gelu":
            g1 = round16(gelu_tanh(x1), d1)
        else:
            g1 = gelu_pk16(x1) if rt["gelu16"] else round16(gelu_formula(x1), d1)
        y = (g1 @ w2.t()).reshape(n, T, 4, 4, C2) + b2
        if mutation == "tanh_gelu":
            g2 = rh(gelu_tanh(y))
        else:
            g2 = gelu_pk16(y) if rt["gelu16"] else rh(gelu_formula(y))
        h = _hyper_rows(inp, lo, lo + chunk)
        hi_ = rh(h)
        hp = hi_ if mutation == "hyper_lo_dropped" else hi_ + rh(h - hi_)
        o = _project(hp, g2)
        if rt["out16"]:
            if mutation == "out16_truncated":
                o = o.float()                                                            # (the fp32 accumulator), its low 13 bits cut off
                o = (o.view(torch.int32) & -8192).view(torch.float32).to(torch.float16).double()
            else:
                o = rh(o)
        outs.append(pixels(o))
    return torch.cat(outs)


def plane_means(err):
    """mean over the pixels of every (prompt, mask) plane: [n, m]"""
    return err.abs().mean(dim=(-1, -2))


# ------------------------------------------------------------------------------------------------------------------- mutations
def _tile(o, p, t0):
    """The [m, 16, 4, 4] block of tile t0 .. t0 + 15 of prompt p in an [n, m, T, 4, 4] tensor."""
    return o[p, :, t0:t0 + TK]


def mutated(inp, mutation, ks=16, grid=None, rt=None):
    """The reference with one defect (fp64 [P, nmask, 256, 256]).  The geometry defects take the launch's key splits and grid; a pixel that
    the defective kernel never stores is 0 here (on the device it is the NaN prefill).  "hyper_lo_dropped" and "out16_truncated" are
    defects of the rounded arithmetic: ``restate`` with the mutation, on route ``rt``."""
    assert mutation in MUTATIONS, mutation
    if mutation in ("hyper_lo_dropped", "out16_truncated"):
        return restate(inp, rt, mutation=mutation)
    P = inp["keys"].shape[0]
    nitems = P * ks
    grid = min(nitems, grid or nitems)
    per = T // ks                                                                        # tokens of a work item
    early = mutation if mutation in ("no_b1", "no_b2", "no_ln_b", "no_eps", "eps_slip", "ln_wrong_64", "blocked_as_row_major", "tanh_gelu") else None
    st = _first_stages(inp, 0, P, early)
    hmut = mutation if mutation in ("mask0_ignored", "hyper_ld_128", "hyper_channels_32") else None
    h = _hyper_rows(inp, 0, P, hmut)
    o = _project(h, st["g2"])                                                            # [P, m, T, 4, 4]
    if mutation == "subpixels_crossed":
        return pixels(o, crossed=True)
    if mutation == "mask_rows_crossed":
        assert inp["nmask"] >= 2
        return pixels(torch.cat([o[:, 1:2], o[:, 0:1], o[:, 2:]], dim=1))
    if mutation == "split_rows_crossed":                                                 # split 2 j writes the rows of split 2 j + 1 and back
        assert ks >= 2
        return pixels(o.reshape(P, -1, ks // 2, 2, per, 4, 4).flip(3).reshape(o.shape))
    good = o
    o = o.clone()
    item_pos = lambda i: (i // ks, (i % ks) * per)                                       # prompt, first token
    if mutation == "last_tile_not_stored":
        for i in range(nitems):
            p, t0 = item_pos(i)
            _tile(o, p, t0 + per - TK).zero_()
    elif mutation == "last_tile_next_base":
        moves = [(i, i + grid) for i in range(nitems - grid) if item_pos(i)[0] != item_pos(i + grid)[0]]
        for i, _ in moves:
            p, t0 = item_pos(i)
            _tile(o, p, t0 + per - TK).zero_()
        for i, j in moves:
            p, t0 = item_pos(i)
            _tile(o, item_pos(j)[0], t0 + per - TK).copy_(_tile(good, p, t0 + per - TK))
    elif mutation == "first_tile_stale_hyper":
        for i in range(nitems - grid):
            (p, _), (p2, t2) = item_pos(i), item_pos(i + grid)
            _tile(o, p2, t2).copy_(_project(h[p:p + 1], st["g2"][p2:p2 + 1, t2:t2 + TK])[0])
    elif mutation == "tile_repeated_at_clamp":                                           # a workgroup's last tile computed on the keys of the one before
        for b in range(grid):
            last = b + ((nitems - 1 - b) // grid) * grid
            p, t0 = item_pos(last)
            _tile(o, p, t0 + per - TK).copy_(_tile(good, p, t0 + per - 2 * TK))
    elif early is None and hmut is None:
        raise AssertionError(mutation)
    return pixels(o)


# ------------------------------------------------------------------------------------------------------------------- generators
def centre_weights(w1, b1, dtype):
    """Every sub-pixel's 64 rows of w1 minus their mean row and b1 minus its mean, in fp64, rounded to the 16-bit type / fp32 afterwards
    (ops.upscale_centre_weights does the same on fp32 values)."""
    w = w1.double().reshape(4, C1, C)
    b = b1.double().reshape(4, C1)
    return (w - w.mean(dim=1, keepdim=True)).reshape(C, C).to(dtype).contiguous(), (b - b.mean(dim=1, keepdim=True)).reshape(C).float().contiguous()


def make(name, dtype, P, dev="cpu", *, centred=True, hyper_ld=128, mask0=1, nmask=3, seed=0):
    """Seeded operands of one launch, drawn on ``dev``: a dict of keys [P, 4096, 256], w1 [256, 256], w2 [128, 64] in ``dtype``, b1 [256], ln_w,
    ln_b [64], b2 [32], hyper [P, 4, hyper_ld] fp32, eps, mask0, nmask, centred (whether w1 / b1 are centred).

    diffuse     the randn operands of tests/test_gpu_kernels.py::test_upscale_fused; every prompt has its own keys and hyper row
    wide        ln_w x 3, ln_b of std 1.5, w2 of std 1 / 6, b2 of std 1.5: the arguments of BOTH GELUs have std ~3.4 and spread over about
                [-9, 9] - the saturating negative tail of the packed-fp16 exponential (2^q flushes to 0 from q < -25), the region around 0,
                large positives
    flat        w1 does not depend on c for the input channels k < 128 and b1 is a small constant per sub-pixel (|b1| <= 1/32), so a token's
                64 channels differ only through its input channels k >= 128.  Of every 8 tokens: token 0 is all zero (u = b1: exactly
                flat), token 1 has only k < 128, scaled by 2^-6 (exactly flat, mean != 0), token 2 has only k >= 128, scaled by 2^-9
                (var ~ eps), the rest are randn.  eps and rsqrt decide the result of the flat groups.  sig - E2 > 0 because
                sig >= sqrt(eps) = 1e-3 while |u| <= ~0.06 in the flat groups: m2 <= 4e-3, so the one-pass loss 80 F m2 <= 2e-8 moves sig
                by <= 2e-8 / (sig - rms E) = 2e-5, and rms(E) + |mu| (CEN: the mean of centred weights' rounding errors) ~ 1e-6.
    large_mean  b1 = 100 + 0.1 randn on activations of std ~1: E[u^2] / var ~ 1e4, the one-pass term of the bound.  Plain weights only.
    hyper_pair  diffuse with hyper = a: fp16 values with 2^-6 <= |a|; the dict also holds hyper_d = a + d, d = +-2^-2 ulp_fp16(a) (an fp16 value,
                subnormal or not, below half an ulp of a: fp16(a + d) = a and the pair's lo half is d exactly)."""
    assert name in GENERATORS and dtype in U, (name, dtype)
    assert not (name == "large_mean" and centred), "large_mean is for the non-centred instantiations"
    dev = torch.device(dev)
    g = torch.Generator(device=dev).manual_seed(1000 * seed + 31 * GENERATORS.index(name) + 5)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=dev)

    w1 = rn(C, C) / 16
    b1 = rn(C1).repeat(4)
    lw, lb = rn(C1) * 0.2 + 1, rn(C1) * 0.3
    w2, b2 = rn(4 * C2, C1) / 8, rn(C2)
    hyper = rn(P, 4, hyper_ld)
    keys = torch.empty(P, T, C, dtype=dtype, device=dev)
    for lo in range(0, P, 64):
        keys[lo:lo + 64] = rn(min(64, P - lo), T, C).to(dtype)
    extra = {}
    if name == "wide":
        lw, lb = lw * 3, rn(C1) * 1.5
        w2, b2 = rn(4 * C2, C1) / 6, rn(C2) * 1.5
    elif name == "flat":
        w1 = w1.reshape(4, C1, C).clone()
        w1[:, :, :128] = w1[:, :1, :128]
        w1 = w1.reshape(C, C)
        b1 = (rn(4).clamp(-2, 2) / 64).repeat_interleave(C1)
        t = torch.arange(T, device=dev)
        keys[:, t % 8 == 0] = 0
        sel = t % 8 == 1
        keys[:, sel, 128:] = 0
        keys[:, sel, :128] = (keys[:, sel, :128].float() * 2.0 ** -6).to(dtype)
        sel = t % 8 == 2
        keys[:, sel, :128] = 0
        keys[:, sel, 128:] = (keys[:, sel, 128:].float() * 2.0 ** -9).to(dtype)
    elif name == "large_mean":
        b1 = (100.0 + 0.1 * rn(C1)).repeat(4)
    elif name == "hyper_pair":
        a = hyper.to(torch.float16).float()
        a = torch.where(a.abs() < 2.0 ** -6, torch.full_like(a, 2.0 ** -6), a)
        ulp = torch.exp2(torch.floor(torch.log2(a.abs())) - 10)
        sign = torch.where(rn(P, 4, hyper_ld) > 0, 1.0, -1.0)
        hyper = a
        extra["hyper_d"] = (a + sign * ulp / 4).contiguous()
    if centred:
        w1, b1 = centre_weights(w1, b1, dtype)
    return dict({"keys": keys, "w1": w1.to(dtype).contiguous(), "b1": b1.float().contiguous(), "ln_w": lw.float(), "ln_b": lb.float(),
                 "w2": w2.to(dtype).contiguous(), "b2": b2.float(), "hyper": hyper.float().contiguous(), "eps": LN_EPS, "mask0": mask0,
                 "nmask": nmask, "centred": bool(centred)}, **extra)


def with_masks(inp, mask0, nmask):
    return dict(inp, mask0=mask0, nmask=nmask)


def with_hyper_ld(inp, ld):
    """The same hyper rows (their first ``ld`` channels) in a buffer of row stride ``ld``."""
    return dict(inp, hyper=inp["hyper"][:, :, :ld].contiguous())


def first_prompts(inp, sel):
    """The operands of the prompts ``sel`` (a slice or an index list) alone."""
    out = dict(inp, keys=inp["keys"][sel].contiguous(), hyper=inp["hyper"][sel].contiguous())
    if "hyper_d" in inp:
        out["hyper_d"] = inp["hyper_d"][sel].contiguous()
    return out
