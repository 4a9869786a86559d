"""Reference, rounding bounds, input families and case table for fine-tuning's fp32 attention kernels (csrc/train.hip: ``attn_fwd`` /
``attn_bwd_q`` / ``attn_bwd_kv`` in their thread-per-row and ``_rowblock`` forms, ``relpos_fwd`` / ``relpos_bwd_q`` / ``relpos_bwd_kv``).
Plain numpy in float64; nothing here touches a device.  tests/test_gpu_train_attention.py runs the table on the GPU,
tests/test_train_attention_host.py runs it (and mutated copies of the source) on the CPU; both go through ``run_case`` / ``check_case``.

THE REFERENCE (``reference``): from the fp32 inputs and the fp32 ``scale`` the kernel is handed,
    s_ij = scale q_i k_j (+ bias_h[i][j / Gw] + bias_w[i][j % Gw]),  P = softmax_j(s),  out = P v,  lse_i = log sum_j exp(s_ij),
    delta_i = dout_i . out_i,  dS_ij = P_ij (dout_i . v_j - delta_i),  dq = scale dS k,  dk = scale dS^T q,  dv = P^T dout,
    dbias_h[i][kh] = sum_kw dS_i(kh,kw),  dbias_w[i][kw] = sum_kh dS_i(kh,kw).

THE BOUNDS are first-order, per element, computed from the inputs and the kernels' operation counts - never from a kernel's output.
u = 2^-24, gamma_n = n u / (1 - n u).
* Logit.  |s^ - s| <= gamma_(D+c) A_ij with A_ij = scale sum_d |q_d k_d| + |bias_h| + |bias_w|.  Forward form (forward, dQ: q is
  scaled first, then D FMAs; rel-pos starts the chain from the rounded bias sum): c = 1, rel-pos 2.  bwd_kv form (D FMAs, then
  ``s * scale``; rel-pos adds the two biases one after the other): c = 1, rel-pos 3.
* Intrinsics.  ``__expf(x)`` is v_exp_f32(x log2 e): the instruction is good to 1 ulp <= E u (E = 2, ``E_INTRINSIC``), the product
  with log2 e and the subtraction that formed x are one rounding of x each: a relative error E (1 + |x|) u at x = s - m.  In the
  online softmax a weight is a PRODUCT of such factors (exp(s - m_t) and one ``a = exp(m_old - m_new)`` per move of the running
  maximum); their arguments telescope to s - m, which is why |x| appears once.  A factor whose argument is 0 is exactly 1; the E u of
  every factor that is not is first order and is what the margin below absorbs together with the second-order terms (two roundings
  per key are counted in the depth, the margin doubles it: room for a 1-ulp factor per key).  ``__logf(l)`` is v_log_f32(l) ln 2:
  (E + 1) u |log l|.
* Softmax weight.  rel. error of P_ij <= 2 max_j(logit error of row i) + E (1 + |x_ij|) u + sum_k P_ik E (1 + |x_ik|) u (numerator;
  the denominator is a P-weighted mean of the same errors).  The backward passes evaluate P = exp(s - lse^) with the FORWARD
  kernel's lse: logit error of the pass's own form + the bound of lse + E (1 + |s - lse|) u.
* Accumulation depth.  Thread-per-row: two roundings per key (``acc * a``, the FMA): 2 Nk (2 Nq for dK / dV).  Row-block:
  2 ceil(N / 256) for the thread's stride loop, the 6-level butterfly, the 3 additions of the four wave sums, the final division, and for
  the forward merge the product ``acc * r`` with r = exp(m - M) itself (1 + E).  dbias_h / dbias_w: Gw / Gh plain additions.
* Propagation.  out = sum_j P_ij v_j over l: weight errors through sum_j P_ij |v_jd|, the accumulation of numerator and denominator,
  the reciprocal and the product.  lse: the P-weighted mean of the weight errors, the depth of l, the logarithm, the final addition.
  delta: D FMAs on the kernel's own out, so the bound of out enters.  dS = P (dP - delta): the errors of P, of the D-FMA dot product
  dP, of delta and of the subtraction; then the depth of the sum over keys (queries) and the final ``* scale``.
* Margin.  Every bound is doubled (second-order terms; see above), as the LayerNorm bound of tests/test_gpu_det_reductions.py is.
E_INTRINSIC: derived (1 ulp per the ISA's statement for v_exp_f32 / v_log_f32) and then confirmed by measurement on the device - see
``E_MEASURED``; it was never fitted to a kernel's output.

FOUR INPUT FAMILIES (``make_case``), seeded:
* ``uniform`` (exact): q = 0 (rel-pos: bias_h = b_i and bias_w = -b_i, constant per row, so both are read and every logit is exactly 0;
  with a sum other than 0 the rounding of m + log N would end the exactness of dv), k / v / dout small integers.  Every exponential is exp(0) = 1 and
  every sum an integer below 2^24: out is the float64 mean bit for bit when the key count is a power of two (within 2 ulp
  otherwise), delta equals dout . out, dv is exact for power-of-two counts, lse is log N to the rounding of ``__logf`` alone.
* ``onehot`` (exact): every query i has ONE key pi(i) whose logit is >= 40 above all others, so P is a permutation-like 0 / 1 matrix to
  e^-40: out[i] must EQUAL v[pi(i)] (non-zero integers) bit for bit - a gather no indexing error survives -, lse the target's logit, dv
  the scatter-add of the dout rows, dq / dk / dbias the leakage alone (dP - delta cancels).  pi covers key 0, the last key, 255 /
  256 / 257, both ends of the short last stride of the row-block loop and the block edges of the thread-per-row kernels; where there
  are fewer queries than such keys the family has several ``variants``.  Plain attention selects by a binary code of the key index
  in q / k (D = 16: +-1 code, exact because scale = 1/4; D = 32: a code whose target products are all 0, because scale is no power of two
  and the forward and bwd_kv forms round a non-zero logit differently).  Rel-pos selects by bias_h = 40 at kh* and bias_w = 40 at kw*
  (row and column neighbours sit at e^-40; Gh != Gw sends a swapped j / Gw, j % Gw to another key) with the same zero-target code in
  q / k.  THE SHIFTED CALL: the backward pass is run a second time with ``out + c`` (one non-zero integer per row) for out, so
  delta moves by dout . c and dS at the target becomes the integer t_i = -dout_i . c_i: dq[i] = scale t_i k[pi(i)], dk the scatter-add of
  scale t_i q_i, dbias_h / dbias_w = t_i at (kh*, kw*) - exact, non-zero gradients.  (The mutation check of the host test found that
  a missing ``* scale`` on dk and a shifted dbias_w column survive the two families without it: there dq / dk / dbias are all ~ 0.)
* ``diffuse``: logits about N(0, 1); checked against the bounds.
* ``peaked``: logits up to about +-60, in three key orders: ``last`` (logits ascend along the keys: the running maximum moves at almost
  every step), ``first`` (it never moves), ``random``; checked against the bounds.
The bounds are checked in the exact families too (they hold for any input).

THE CASE TABLE (``PLAIN_SHAPES`` x D in (16, 32), ``RELPOS_SHAPES`` x D in (64, 80)), BH = 2 so that a wrong batch stride shows: the
smallest shapes that reach every branch of the launchers' route conditions (``Nq <= 64 && Nk >= 1024`` and its mirror) on both sides,
short last strides, the block edges of the 128-thread kernels, Gw at the LDS limit with one full and with a partial second
block, Gh > 64.
"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
E_INTRINSIC = 2.0
# Measured on an MI355X, in units of u, by test_intrinsics_are_within_the_constant_the_bounds_use (cases whose float64 value isolates the
# intrinsic): ``__expf`` 1.09 against E_INTRINSIC = 2 (x in [0, 80], after the 3 u of the surrounding operations); ``__logf`` with its
# product by ln 2: 2.09 against E_INTRINSIC + 1 = 3.  The derived constant holds, so it stays as derived.
E_MEASURED = {"expf": 1.09, "logf": 2.09}
FLOOR = 2.0 ** -100                 # absolute slack: exponentials below 2^-126 are flushed to zero
MARGIN = 40.0                       # one-hot: the target's logit is at least this far above every other
LEAK = math.exp(-MARGIN)

BH = 2
PLAIN_DIMS = (16, 32)
RELPOS_DIMS = (64, 80)
# (Nq, Nk): row-block forward / dQ; just outside it; row-block dK / dV; just outside; thread-per-row block edges
PLAIN_SHAPES = [(1, 1024), (3, 1025), (64, 1279), (65, 1024), (64, 1023),
                (1024, 1), (1025, 3), (1279, 64), (1024, 65), (1023, 64),
                (1, 1), (127, 5), (128, 128), (129, 130)]
ROWBLOCK_SHAPES = [(1, 1024), (3, 1025), (64, 1279), (1024, 1), (1025, 3), (1279, 64)]
# (Gh, Gw)
RELPOS_SHAPES = [(1, 1), (2, 64), (3, 64), (70, 2), (5, 9), (8, 16), (14, 14)]
PEAK_ORDERS = ("last", "first", "random")
OUTPUTS = ("out", "lse", "delta", "dq", "dk", "dv", "dbias_h", "dbias_w")


def gamma(n):
    return n * U / (1 - n * U)


def q_rows_route(Nq, Nk):
    """msam_attention_forward / _backward: a workgroup per query row for (out, lse) and (delta, dQ)."""
    return Nq <= 64 and Nk >= 1024


def k_rows_route(Nq, Nk):
    """msam_attention_backward: a workgroup per key row for (dK, dV)."""
    return Nk <= 64 and Nq >= 1024


def depth(rowblock, n, merge_exp=False):
    """Roundings on the way of one term through a sum over n keys (queries)."""
    if not rowblock:
        return 2 * n
    return 2 * ((n + 255) // 256) + 6 + 3 + 1 + ((1 + E_INTRINSIC) if merge_exp else 0)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------

def _special_keys(n, stride):
    """Keys an indexing error is likely to lose: both ends, the edges of the first stride and of the short last one."""
    last0 = ((n - 1) // stride) * stride
    ks = [0, n - 1, stride - 1, stride, stride + 1, last0 - 1, last0, n - 2]
    out = []
    for x in ks:
        if 0 <= x < n and x not in out:
            out.append(x)
    return out


def onehot_variants(op, Nq, Nk):
    """How many one-hot cases it takes for pi to reach every special key (BH * Nq targets per case)."""
    sp = len(_special_keys(Nk, 256 if op == "plain" else 128))
    return max(1, -(-sp // (BH * Nq)))


def _nonzero_ints(rng, shape, hi):
    return (rng.integers(1, hi + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


def _code_bits(n):
    return max(1, int(n - 1).bit_length())


def _signed_code(idx, bits):
    return (2.0 * ((idx[..., None] >> np.arange(bits)) & 1) - 1.0).astype(np.float32)


def _onehot_qk(rng, pi, Nk, D, G, signed):
    """q [BH, Nq, D], k [BH, Nk, D] with q_i k_j largest at j = pi(i).  signed: k = +-1 code of j, q = G x code of pi: q k = G (bits -
    2 hamming).  Otherwise k = (code, complement of the code) in 0 / 1 and q = -G where pi's (code, complement) is 0: q k = -G hamming,
    every product of the target pair is exactly 0."""
    bits = _code_bits(Nk)
    keys = np.arange(Nk)
    q = np.zeros(pi.shape + (D,), np.float32)
    k = np.zeros((pi.shape[0], Nk, D), np.float32)
    if signed:
        assert bits <= D
        k[:, :, :bits] = _signed_code(keys, bits)[None]
        q[:, :, :bits] = G * _signed_code(pi, bits)
    else:
        assert 2 * bits <= D
        kb = ((keys[:, None] >> np.arange(bits)) & 1).astype(np.float32)
        pb = ((pi[..., None] >> np.arange(bits)) & 1).astype(np.float32)
        k[:, :, :bits], k[:, :, bits:2 * bits] = kb[None], 1.0 - kb[None]
        q[:, :, :bits], q[:, :, bits:2 * bits] = -G * (1.0 - pb), -G * pb
    return q, k


def make_case(op, shape, D, family, variant=0):
    """One seeded case: SimpleNamespace with the fp32 inputs q, k, v, dout (bias_h, bias_w for ``relpos``) and, for ``onehot``, pi
    [BH, Nq] and the shift c [BH, Nq, D] of the second backward call."""
    if op == "plain":
        Nq, Nk = shape
        Gh = Gw = None
    else:
        Gh, Gw = shape
        Nq = Nk = Gh * Gw
    seed = [{"plain": 1, "relpos": 2}[op], shape[0], shape[1], D, ("uniform", "onehot", "diffuse", "peaked").index(family.split(":")[0]),
            variant, PEAK_ORDERS.index(family.split(":")[1]) if ":" in family else 0]
    rng = np.random.default_rng(seed)
    scale = np.float32(D ** -0.5)
    c = SimpleNamespace(op=op, shape=tuple(shape), BH=BH, Nq=Nq, Nk=Nk, D=D, Gh=Gh, Gw=Gw, scale=scale, family=family, variant=variant,
                        pi=None, shift=None, bias_h=None, bias_w=None)
    fam = family.split(":")[0]
    if fam == "uniform":
        c.q = np.zeros((BH, Nq, D), np.float32)
        c.k = rng.integers(-3, 4, (BH, Nk, D)).astype(np.float32)
        c.v = rng.integers(-4, 5, (BH, Nk, D)).astype(np.float32)
        c.dout = rng.integers(-3, 4, (BH, Nq, D)).astype(np.float32)
        if op == "relpos":
            b = rng.integers(1, 4, (BH, Nq, 1))                       # bias_h = b_i, bias_w = -b_i: read, and every logit is exactly 0
            c.bias_h = np.repeat(b, Gh, 2).astype(np.float32)
            c.bias_w = np.repeat(-b, Gw, 2).astype(np.float32)
    elif fam == "onehot":
        sp = _special_keys(Nk, 256 if op == "plain" else 128)
        if op == "relpos":                                             # + the ends of the first grid row, the start of the last one
            sp += [x for x in (Gw - 1, Gw, Nk - Gw) if 0 <= x < Nk and x not in sp]
        pi = rng.integers(0, Nk, (BH, Nq))
        flat = pi.reshape(-1)
        n = BH * Nq
        for t in range(min(n, len(sp))):                                # spread the special keys over both batches and the variants
            flat[t * (n // len(sp)) if n >= len(sp) else t] = sp[(t + variant * n) % len(sp)]
        c.pi = pi = flat.reshape(BH, Nq)
        if op == "plain":
            c.q, c.k = _onehot_qk(rng, pi, Nk, D, 96.0 if D == 16 else 256.0, signed=(D == 16))
        else:
            c.q, c.k = _onehot_qk(rng, pi, Nk, D, 8.0, signed=False)
            c.bias_h = np.zeros((BH, Nq, Gh), np.float32)
            c.bias_w = np.zeros((BH, Nq, Gw), np.float32)
            np.put_along_axis(c.bias_h, (pi // Gw)[..., None], np.float32(MARGIN), 2)
            np.put_along_axis(c.bias_w, (pi % Gw)[..., None], np.float32(MARGIN), 2)
        c.v = _nonzero_ints(rng, (BH, Nk, D), 8)
        c.dout = _nonzero_ints(rng, (BH, Nq, D), 3)
        c.shift = np.zeros((BH, Nq, D), np.float32)
        np.put_along_axis(c.shift, rng.integers(0, D, (BH, Nq, 1)), _nonzero_ints(rng, (BH, Nq, 1), 2), 2)
    elif fam == "diffuse":
        c.q, c.k, c.v = (rng.standard_normal((BH, n, D)).astype(np.float32) for n in (Nq, Nk, Nk))
        c.dout = rng.standard_normal((BH, Nq, D)).astype(np.float32)
        if op == "relpos":
            c.bias_h = (0.5 * rng.standard_normal((BH, Nq, Gh))).astype(np.float32)
            c.bias_w = (0.5 * rng.standard_normal((BH, Nq, Gw))).astype(np.float32)
    elif fam == "peaked":
        # s_ij ~ 60 alpha_i beta_j + noise: alpha in [0.5, 1], beta spread over [-1, 1] in the family's key order.  The noise of the
        # ordered forms stays below the spacing of the logits (120 / Nk), so that the order is the logits' order
        order = family.split(":")[1]
        noise = D ** 0.25 * (0.3 if order == "random" else 0.01)
        g = rng.standard_normal((BH, 1, D))
        g /= np.linalg.norm(g, axis=-1, keepdims=True)
        beta = np.linspace(-1.0, 1.0, Nk) if Nk > 1 else np.ones(1)
        beta = np.stack([{"last": beta, "first": beta[::-1], "random": rng.permutation(beta)}[order] for _ in range(BH)])
        alpha = rng.uniform(0.5, 1.0, (BH, Nq, 1))
        amp = math.sqrt(60.0 / float(scale))
        c.q = (amp * alpha * g + noise * rng.standard_normal((BH, Nq, D))).astype(np.float32)
        c.k = (amp * beta[..., None] * g + noise * rng.standard_normal((BH, Nk, D))).astype(np.float32)
        c.v = rng.standard_normal((BH, Nk, D)).astype(np.float32)
        c.dout = rng.standard_normal((BH, Nq, D)).astype(np.float32)
        if op == "relpos":
            if order == "random":
                c.bias_h = (2.0 * rng.standard_normal((BH, Nq, Gh))).astype(np.float32)
                c.bias_w = (2.0 * rng.standard_normal((BH, Nq, Gw))).astype(np.float32)
            else:                                                       # bias_h follows the order of the keys, bias_w stays below the spacing
                ramp = np.linspace(-3.0, 3.0, Gh) if Gh > 1 else np.zeros(1)
                c.bias_h = (alpha * (ramp if order == "last" else ramp[::-1]) + 0.01 * rng.standard_normal((BH, Nq, Gh))).astype(np.float32)
                c.bias_w = (0.01 * rng.standard_normal((BH, Nq, Gw))).astype(np.float32)
    else:
        raise ValueError(family)
    return c


def case_list(op, exact=True, bounded=True):
    """The table: every shape x head dim with its families.  Both exact families and both kinds of bounded family run on every shape."""
    shapes, dims = (PLAIN_SHAPES, PLAIN_DIMS) if op == "plain" else (RELPOS_SHAPES, RELPOS_DIMS)
    out = []
    for shape in shapes:
        for D in dims:
            Nq, Nk = shape if op == "plain" else (shape[0] * shape[1],) * 2
            if exact:
                out.append((op, shape, D, "uniform", 0))
                out += [(op, shape, D, "onehot", r) for r in range(onehot_variants(op, Nq, Nk))]
            if bounded:
                out.append((op, shape, D, "diffuse", 0))
                out += [(op, shape, D, "peaked:" + o, 0) for o in PEAK_ORDERS]
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# reference and bounds
# ------------------------------------------------------------------------------------------------------------------------------

def _bias(c, bh, bw):
    """[BH, Nq, Gh] + [BH, Nq, Gw] -> [BH, Nq, Gh * Gw] (key j = kh * Gw + kw)."""
    return (bh[:, :, :, None] + bw[:, :, None, :]).reshape(c.BH, c.Nq, c.Nk)


def reference(c):
    """float64 values ``ref[name]`` and first-order bounds ``bound[name]`` for every output of the forward and the backward pass."""
    relpos = c.op == "relpos"
    D, Nq, Nk = c.D, c.Nq, c.Nk
    q, k, v, do = (a.astype(np.float64) for a in (c.q, c.k, c.v, c.dout))
    scale = float(c.scale)
    kT, vT = k.transpose(0, 2, 1), v.transpose(0, 2, 1)
    S = scale * (q @ kT)
    A = scale * (np.abs(q) @ np.abs(kT))
    if relpos:
        bh, bw = c.bias_h.astype(np.float64), c.bias_w.astype(np.float64)
        S = S + _bias(c, bh, bw)
        A = A + _bias(c, np.abs(bh), np.abs(bw))
    m = S.max(-1, keepdims=True)
    X = S - m
    p = np.exp(X)
    l = p.sum(-1, keepdims=True)
    P = p / l
    lse = m + np.log(l)
    out = P @ v
    delta = (do * out).sum(-1, keepdims=True)
    dP = do @ vT
    T = dP - delta
    dS = P * T
    ref = {"out": out, "lse": lse[..., 0], "delta": delta[..., 0], "dq": scale * (dS @ k), "dk": scale * (dS.transpose(0, 2, 1) @ q),
           "dv": P.transpose(0, 2, 1) @ do}
    # ---- bounds
    E = E_INTRINSIC
    rb_q = (not relpos) and q_rows_route(Nq, Nk)
    rb_k = (not relpos) and k_rows_route(Nq, Nk)
    e_f = gamma(D + (2 if relpos else 1)) * A
    e_k = gamma(D + (3 if relpos else 1)) * A
    e_row = e_f.max(-1, keepdims=True)
    I_f = E * (1 + np.abs(X)) * U
    I_bar = (P * I_f).sum(-1, keepdims=True)
    relP = 2 * e_row + I_f + I_bar
    g_f = gamma(depth(rb_q, Nk, merge_exp=True))
    av, ak, aq, ado = np.abs(v), np.abs(k), np.abs(q), np.abs(do)
    r_out = (P * relP) @ av + g_f * (P @ av + np.abs(out)) + 2 * U * np.abs(out)
    r_lse = e_row + I_bar + g_f + (E + 1) * U * np.abs(np.log(l)) + U * np.abs(lse)
    r_delta = (ado * r_out).sum(-1, keepdims=True) + gamma(D) * np.abs(do * out).sum(-1, keepdims=True)
    I_b = E * (1 + np.abs(S - lse)) * U
    relP_q = e_f + r_lse + I_b
    relP_k = e_k + r_lse + I_b
    r_T = gamma(D) * (ado @ av.transpose(0, 2, 1)) + r_delta + U * np.abs(T)
    r_dS_q = P * ((relP_q + U) * np.abs(T) + r_T)
    r_dS_k = P * ((relP_k + U) * np.abs(T) + r_T)
    adS = np.abs(dS)
    g_q, g_k = gamma(depth(rb_q, Nk)), gamma(depth(rb_k, Nq))
    raw = {"out": r_out, "lse": r_lse[..., 0], "delta": r_delta[..., 0],
           "dq": scale * (r_dS_q @ ak + g_q * (adS @ ak)) + U * np.abs(ref["dq"]),
           "dk": scale * (r_dS_k.transpose(0, 2, 1) @ aq + g_k * (adS.transpose(0, 2, 1) @ aq)) + U * np.abs(ref["dk"]),
           "dv": (P * relP_k).transpose(0, 2, 1) @ ado + g_k * (P.transpose(0, 2, 1) @ ado)}
    if relpos:
        g4 = (c.BH, Nq, c.Gh, c.Gw)
        ref["dbias_h"], ref["dbias_w"] = dS.reshape(g4).sum(3), dS.reshape(g4).sum(2)
        raw["dbias_h"] = r_dS_q.reshape(g4).sum(3) + gamma(c.Gw) * adS.reshape(g4).sum(3)
        raw["dbias_w"] = r_dS_q.reshape(g4).sum(2) + gamma(c.Gh) * adS.reshape(g4).sum(2)
    bound = {n: 2 * b + FLOOR for n, b in raw.items()}
    extra = SimpleNamespace(S=S, m=m[..., 0], l=l[..., 0], dP=dP)
    return ref, bound, extra


# ------------------------------------------------------------------------------------------------------------------------------
# running a case through a backend, and the assertions
# ------------------------------------------------------------------------------------------------------------------------------

def run_case(backend, c):
    """backend.forward(c) -> (out, lse); backend.backward(c, out, lse) -> dict(dq, dk, dv, delta[, dbias_h, dbias_w]); all numpy fp32.
    The one-hot family runs the backward pass a second time on ``out + c.shift`` (keys ``shift_*``)."""
    out, lse = backend.forward(c)
    got = {"out": out, "lse": lse}
    got.update(backend.backward(c, out, lse))
    if c.shift is not None:
        got.update({"shift_" + n: a for n, a in backend.backward(c, out + c.shift, lse).items()})
    return got


RATIOS = {}             # (backend name, op, output) -> largest err / bound seen by check_case


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _is_pow2(n):
    return n & (n - 1) == 0


def check_case(c, got, tag="host"):
    """Every assertion of the case's family -> list of (kind, output, message) for those that FAIL; kind is ``exact`` (an equality or a
    derived leakage bound of an exact family) or ``bound`` (a rounding bound)."""
    ref, bound, ex = reference(c)
    fails = []

    def fail(kind, name, msg):
        fails.append((kind, name, f"{c.op} {c.shape} D={c.D} {c.family}/{c.variant}: {name}: {msg}"))

    g64 = {n: a.astype(np.float64) for n, a in got.items()}
    for n, a in got.items():
        if not np.isfinite(a).all():
            fail("exact" if c.family in ("uniform", "onehot") else "bound", n, "not finite (or not written)")
    # ---- the rounding bounds: every family
    for n in OUTPUTS:
        if n not in ref:
            continue
        err = np.abs(g64[n] - ref[n])
        with np.errstate(invalid="ignore"):
            ratio = float(np.nan_to_num(err / bound[n], nan=np.inf).max())
        key = (tag, c.op, n)
        if np.isfinite(ratio):
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        if not ratio <= 1.0:
            at = np.unravel_index(np.argmax(np.nan_to_num(err / bound[n], nan=np.inf)), err.shape)
            fail("bound", n, f"err / bound = {ratio:.3g} at {at} (err {err[at]:.3g}, bound {bound[n][at]:.3g})")
    fam = c.family.split(":")[0]
    D, Nq, Nk = c.D, c.Nq, c.Nk
    do, v = c.dout.astype(np.float64), c.v.astype(np.float64)
    if fam == "uniform":
        assert float(np.abs(v).sum(1).max()) < 2 ** 24 and float(np.abs(do).sum(1).max()) < 2 ** 24
        mean = np.broadcast_to(v.sum(1, keepdims=True) / Nk, (c.BH, Nq, D))      # integer sums: exact; one division
        if _is_pow2(Nk):
            if not np.array_equal(g64["out"], mean):
                fail("exact", "out", f"not the mean bit for bit (max diff {np.abs(g64['out'] - mean).max():.3g})")
            if not np.array_equal(g64["delta"], (do * mean).sum(-1)):
                fail("exact", "delta", f"not dout . out exactly (max diff {np.abs(g64['delta'] - (do * mean).sum(-1)).max():.3g})")
            dv = np.broadcast_to(do.sum(1, keepdims=True) / Nk, (c.BH, Nk, D))
            if not np.array_equal(g64["dv"], dv):
                fail("exact", "dv", f"not sum_i dout_i / Nk exactly (max diff {np.abs(g64['dv'] - dv).max():.3g})")
        else:
            e = np.abs(g64["out"] - mean)
            if not (e <= 2 * _ulp32(mean)).all():
                fail("exact", "out", f"more than 2 ulp from the mean (max diff {e.max():.3g})")
            own = (do * g64["out"]).sum(-1)                               # the kernel's D FMAs on its own out
            e = np.abs(g64["delta"] - own)
            if not (e <= gamma(D) * np.abs(do * g64["out"]).sum(-1)).all():
                fail("exact", "delta", f"not dout . out to its own D roundings (max diff {e.max():.3g})")
        want = ex.m + math.log(Nk)                                        # l = Nk exactly: only __logf and the final addition round
        e = np.abs(g64["lse"] - want)
        if not (e <= 2 * ((E_INTRINSIC + 1) * U * math.log(Nk) + U * np.abs(want))).all():
            fail("exact", "lse", f"not m + log Nk to the rounding of the logarithm (max diff {e.max():.3g})")
    elif fam == "onehot":
        pi = c.pi
        S = ex.S
        tgt = np.take_along_axis(S, pi[..., None], 2)
        others = S.copy()
        np.put_along_axis(others, pi[..., None], -np.inf, 2)
        if Nk > 1:                                                        # the family's premise, with room for the fp32 logit error
            assert float((tgt[..., 0] - others.max(-1)).min()) >= MARGIN + 0.5, "one-hot inputs: margin below 40"
        bidx = np.arange(c.BH)[:, None]
        if not np.array_equal(got["out"], c.v[bidx, pi]):
            bad = np.argwhere((got["out"] != c.v[bidx, pi]).any(-1))
            fail("exact", "out", f"out[i] != v[pi(i)] at {len(bad)} rows, first (bh, i) = {tuple(bad[0])} with pi = {pi[tuple(bad[0])]}")
        if not np.array_equal(g64["lse"], tgt[..., 0]):
            fail("exact", "lse", f"not the target's logit (max diff {np.abs(g64['lse'] - tgt[..., 0]).max():.3g})")
        if not np.array_equal(g64["delta"], (do * v[bidx, pi]).sum(-1)):
            fail("exact", "delta", "not dout . v[pi]")
        onehot = np.zeros((c.BH, Nq, Nk))
        np.put_along_axis(onehot, pi[..., None], 1.0, 2)
        dv_ideal = onehot.transpose(0, 2, 1) @ do                         # scatter-add of the dout rows (integers: exact)
        amax = lambda a: float(np.abs(a).max())
        scale = float(c.scale)
        for pre, shift in (("", None), ("shift_", c.shift.astype(np.float64))):
            # t_i = dS at the target = dout_i . v_pi - dout_i . (v_pi + c_i); elsewhere |dS| <= e^-40 max |dP - delta|
            t = np.zeros((c.BH, Nq)) if shift is None else -(do * shift).sum(-1)
            dl = (do * (v[bidx, pi] + (0 if shift is None else shift))).sum(-1)
            Tmax = amax(ex.dP - dl[..., None])
            ideal = {"dv": dv_ideal,
                     "dq": (t[..., None] * c.k.astype(np.float64)[bidx, pi] * scale).astype(np.float32).astype(np.float64),
                     "dk": ((onehot * t[..., None]).transpose(0, 2, 1) @ c.q.astype(np.float64) * scale).astype(np.float32).astype(np.float64)}
            leak = {"dv": Nq * LEAK * amax(do), "dq": scale * Nk * LEAK * Tmax * amax(c.k), "dk": scale * Nq * LEAK * Tmax * amax(c.q)}
            if c.op == "relpos":
                ideal["dbias_h"], ideal["dbias_w"] = np.zeros((c.BH, Nq, c.Gh)), np.zeros((c.BH, Nq, c.Gw))
                np.put_along_axis(ideal["dbias_h"], (pi // c.Gw)[..., None], t[..., None], 2)
                np.put_along_axis(ideal["dbias_w"], (pi % c.Gw)[..., None], t[..., None], 2)
                leak["dbias_h"], leak["dbias_w"] = c.Gw * LEAK * Tmax, c.Gh * LEAK * Tmax
            if shift is not None and not np.array_equal(g64[pre + "delta"], dl):
                fail("exact", pre + "delta", "not dout . (out + c)")
            for n, w in ideal.items():
                e = np.abs(g64[pre + n] - w)
                if not (e <= leak[n]).all():
                    at = np.unravel_index(np.argmax(e), e.shape)
                    fail("exact", pre + n, f"off the exact gather / scatter by {e[at]:.3g} at {at} (leakage bound {leak[n]:.3g})")
    return fails


def format_ratios(tag):
    rows = sorted((op, n, r) for (t, op, n), r in RATIOS.items() if t == tag)
    return "\n".join(f"  {tag:6s} {op:6s} {n:8s} max err / bound = {r:.3f}" for op, n, r in rows)
