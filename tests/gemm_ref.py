"""Harness, operand generators and references for the device pin of the GEMM family (csrc/gemm.hip: ``msam_gemm_bf16`` with its 128 x 128,
256 x 256, fused-LayerNorm, fp8 and split-K launches, and ``msam_gemm_group_bf16``).  Pure Python / torch: the same code drives the GPU
library (tests/test_gpu_gemm_routes.py) and the host-compiled one (tests/test_gemm_routes_host.py).

* ``call`` / ``call_group`` fill ``_lib.GemmParams`` directly, so every field of the ABI is reachable (leading dimensions larger than the
  logical width, any table geometry, 16-bit residuals of either type, the LayerNorm side outputs, fp8 scales, split-K).  Every buffer is a
  logical matrix inside a larger allocation whose row padding and 64 guard elements in front and behind hold a NaN sentinel; after the
  call the inputs must be unchanged bit for bit and the sentinels of the outputs must still be there.  A refused call (status != 0) must
  leave its outputs untouched altogether.
* ``route_taken`` reports the profile family a launch recorded (0 = gemm256_kernel, 5 = gemm_kernel / gemm_ln_kernel / the grouped
  launch, None = no record: split-K), so a test knows which kernel a shape really took.
* ``exact_case``: integer operands in [-3, 3] and integer bias / table / residual (power-of-two scales for fp8).  Every product and every
  partial sum is an integer far below 2^24 in ANY accumulation order and in any arithmetic an MFMA may use internally, so the fp32 result
  must EQUAL the exact one, and a 16-bit output must equal the round-to-nearest-even cast of it - bit for bit.  The bias magnitudes put
  the results where the 16-bit type's spacing is at least 2 (above 512 for bf16, above 2048 for fp16): the generator asserts on its own
  reference that >= 25 % of the results are inexact in the 16-bit type and >= 1 % are exact ties, so truncation, double rounding and
  round-half-away all show.  Rows of A, rows of W and k-columns are pairwise distinct (asserted), so an index swap changes the result.
* ``random_case``: the Gaussian operands of tests/test_gpu_kernels.py, for realistic magnitudes.
* ``expected`` turns a case into the outputs of its launch (plain, q / k / v, k / vT, hi | lo | hi); its ``defect`` argument produces the
  result a subtly wrong kernel would give - tests/test_gemm_routes_host.py shows that each defect breaks bit equality on the generators."""
import ctypes as C
import math
import os
import re

import numpy as np
import torch

GUARD = 64
F32, BF16, FP8, F16 = 1, 2, 3, 4
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
GROUP_MAX = 5                                              # include/msam_hip.h MSAM_GEMM_GROUP_MAX
FP8_T = torch.float8_e4m3fn
_CODE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, FP8_T: FP8}
_SENTINEL = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, FP8_T: 0x7F}       # quiet NaNs
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
THRESH16 = {torch.bfloat16: 512, torch.float16: 2048}      # |result| above this: the type's spacing is >= 2


def bits(t):
    """The tensor's storage as integers of the element size (a view for contiguous tensors)."""
    return t.detach().contiguous().view(_INT[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def _pattern(dtype):
    return _SENTINEL[dtype]


class Padded:
    """A logical [rows, cols] matrix inside GUARD + rows * ld + GUARD elements; everything outside the logical part is a NaN sentinel."""

    def __init__(self, rows, cols, ld, dtype, dev, data=None):
        ld = max(int(ld), cols)
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.flat = torch.empty(2 * GUARD + rows * ld, dtype=dtype, device=dev)
        bits(self.flat).fill_(_pattern(dtype))
        self.body = self.flat[GUARD:GUARD + rows * ld].view(rows, ld)
        self.view = self.body[:, :cols]
        if data is not None:
            assert tuple(data.shape) == (rows, cols) and data.dtype == dtype, (tuple(data.shape), data.dtype, rows, cols, dtype)
            self.view.copy_(data.to(dev))
        self.before = bits(self.flat).clone()

    def ptr(self):
        return self.view.data_ptr()

    def unchanged(self):
        return bool(torch.equal(bits(self.flat), self.before))

    def padding_intact(self):
        b, pat = bits(self.flat), _pattern(self.dtype)
        ok = bool((b[:GUARD] == pat).all()) and bool((b[-GUARD:] == pat).all())
        if self.ld > self.cols:
            ok = ok and bool((b[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.cols:] == pat).all())
        return ok

    def logical(self):
        return self.view.clone()


def _vec(t, dev):
    return None if t is None else Padded(1, t.numel(), t.numel(), t.dtype, dev, t.reshape(1, -1))


class Prepared:
    """One product: the filled ``GemmParams``, its padded inputs and sentinel-filled outputs."""

    def __init__(self, dev, A, W, *, lda=None, ldw=None, bias=None, table=None, table_cols=None, table_ld=None, table_rows=None,
                 resid=None, resid_rows=0, ldr=None, inplace=False, act=ACT_NONE, out_dtype=torch.float32, ldc=None, out_mode=0,
                 heads=0, head_dim=0, tokens=0, use_glds=0, ln_mode=0, ln_w=None, ln_b=None, ln_eps=1e-5, ln_add=None, ln_out_a=False,
                 ln_out_b=False, row_scale=None, col_scale=None, split_k=0, a_dtype=None, M=None, N=None, K=None):
        from micro_sam_amd import _lib
        self.dev = dev
        Ml, Kl = A.shape
        Nl = W.shape[0]
        M, N, K = M or Ml, N or Nl, K or Kl
        self.M, self.N, self.K, self.out_mode, self.inplace = M, N, K, out_mode, inplace
        self.inputs, self.outputs = [], {}
        p = _lib.GemmParams()
        a = Padded(Ml, Kl, lda or Kl, A.dtype, dev, A)
        w = Padded(Nl, Kl, ldw or Kl, W.dtype, dev, W)
        self.inputs += [a, w]
        p.A, p.lda, p.W, p.ldw, p.M, p.N, p.K = a.ptr(), lda or Kl, w.ptr(), ldw or Kl, M, N, K
        p.a_dtype = a_dtype if a_dtype is not None else (0 if A.dtype == torch.bfloat16 else _CODE[A.dtype])
        op16 = torch.float16 if A.dtype == torch.float16 else torch.bfloat16

        def vec(t):
            v = _vec(t, dev)
            if v is not None:
                self.inputs.append(v)
            return None if v is None else v.ptr()
        p.bias = vec(bias)
        if table is not None:
            tb = Padded(table.shape[0], table.shape[1], table_ld or table.shape[1], table.dtype, dev, table)
            self.inputs.append(tb)
            p.table, p.table_rows, p.table_ld = tb.ptr(), table.shape[0] if table_rows is None else table_rows, table_ld or table.shape[1]
            p.table_cols = table.shape[1] if table_cols is None else table_cols
        out_cols = 3 * N if out_mode == 3 else N
        ldc = out_cols if ldc is None else ldc
        if out_mode in (0, 3):
            if inplace:
                assert resid is not None and resid.dtype == out_dtype and tuple(resid.shape) == (M, N) and not resid_rows
                o = Padded(M, out_cols, ldc, out_dtype, dev, resid)
                p.resid, p.resid_dtype, p.resid_rows, p.ldr = o.ptr(), _CODE[resid.dtype], 0, ldc
            else:
                o = Padded(M, out_cols, ldc, out_dtype, dev)
            self.outputs["out"] = o
            p.out = o.ptr()
        p.out_dtype, p.ldc, p.out_mode = _CODE[out_dtype], ldc, out_mode
        if resid is not None and not inplace:
            r = Padded(resid.shape[0], resid.shape[1], ldr or resid.shape[1], resid.dtype, dev, resid)
            self.inputs.append(r)
            p.resid, p.resid_dtype, p.resid_rows, p.ldr = r.ptr(), _CODE[resid.dtype], resid_rows, ldr or resid.shape[1]
        p.act = act
        self.shapes = {}
        if out_mode == 1:
            B = M // tokens
            for nm in ("q", "k", "v"):
                self.outputs[nm] = Padded(1, B * heads * tokens * head_dim, 0, out_dtype, dev)
                self.shapes[nm] = (B, heads, tokens, head_dim)
            p.q, p.k, p.v = (self.outputs[nm].ptr() for nm in ("q", "k", "v"))
        elif out_mode == 2:
            B = M // tokens
            self.outputs["k"] = Padded(M, 128, 128, out_dtype, dev)
            self.outputs["v"] = Padded(1, B * 128 * tokens, 0, out_dtype, dev)
            self.shapes["v"] = (B, 128, tokens)
            p.k, p.v = self.outputs["k"].ptr(), self.outputs["v"].ptr()
        p.heads, p.head_dim, p.tokens = heads, head_dim, tokens
        p.use_glds, p.split_k = use_glds, split_k
        p.ln_mode, p.ln_eps = ln_mode, ln_eps
        p.ln_w, p.ln_b, p.ln_add = vec(ln_w), vec(ln_b), vec(None if ln_add is None else ln_add.reshape(-1))
        for nm, want in (("out_a", ln_out_a), ("out_b", ln_out_b)):
            if want:
                self.outputs[nm] = Padded(M, 256, 256, op16, dev)
                setattr(p, "ln_" + nm, self.outputs[nm].ptr())
        p.row_scale, p.col_scale = vec(row_scale), vec(col_scale)
        self.p = p

    def finish(self, status, what):
        """Checks the sentinels and the inputs; returns the outputs (clones of the logical parts) with ``status``."""
        from micro_sam_amd import _lib
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        res = Result()
        res.status = status
        res.error = _lib.load().msam_last_error().decode("utf-8", "replace") if status else ""
        for i, b in enumerate(self.inputs):
            assert b.unchanged(), f"{what}: input buffer {i} (or its padding) was written"
        for nm, o in self.outputs.items():
            if status != 0:
                assert o.unchanged(), f"{what}: refused (status {status}) but output {nm} was written"
            else:
                assert o.padding_intact(), f"{what}: output {nm}: padding or guard elements were written"
            t = o.logical()
            setattr(res, nm, t.reshape(self.shapes[nm]) if nm in self.shapes else t)
        return res


class Result:
    status = 0
    error = ""
    out = q = k = v = out_a = out_b = None

    def tensors(self):
        return {nm: getattr(self, nm) for nm in ("out", "q", "k", "v", "out_a", "out_b") if getattr(self, nm) is not None}


def call(dev, A, W, expect_ok=True, **kw):
    """One ``msam_gemm_bf16`` launch of the logical operands A [M, K], W [N, K] (16-bit or fp8 e4m3); see ``Prepared`` for the fields."""
    from micro_sam_amd import _lib
    pr = Prepared(dev, A, W, **kw)
    status = _lib.load().msam_gemm_bf16(C.byref(pr.p), _lib.stream_ptr())
    res = pr.finish(status, "msam_gemm_bf16")
    if expect_ok:
        assert status == 0, (status, res.error)
    return res


def call_group(dev, items, expect_ok=True, n=None):
    """One ``msam_gemm_group_bf16`` launch; ``items`` = dicts of ``call``'s arguments (A, W and keywords).  ``n`` overrides the count
    handed to the library (argument tests).  Returns (status, [Result per item])."""
    from micro_sam_amd import _lib
    prs = [Prepared(dev, **it) for it in items]
    arr = (_lib.GemmParams * max(len(prs), 1))(*[pr.p for pr in prs])
    status = _lib.load().msam_gemm_group_bf16(C.cast(arr, C.c_void_p), len(prs) if n is None else n, _lib.stream_ptr())
    res = [pr.finish(status, "msam_gemm_group_bf16") for pr in prs]
    if expect_ok:
        assert status == 0, (status, res[0].error if res else "")
    return status, res


def route_taken(fn):
    """Runs ``fn()`` with the library's launch profile on and returns (fn's result, family): the family of the ONE launch the call
    recorded - 0 = gemm256_kernel, 5 = gemm_kernel / gemm_ln_kernel / grouped - or None if it recorded none (split-K launches are not
    profiled).  ``msam_profile_enable`` clears the record, ``msam_profile_collect_family`` reads and clears it."""
    from micro_sam_amd import _lib
    lib = _lib.load()
    n = (C.c_int32 * _lib.PROFILE_FAMILIES)()
    ms, fl, by = ((C.c_double * _lib.PROFILE_FAMILIES)() for _ in range(3))
    _lib.check(lib.msam_profile_enable(1), "msam_profile_enable")
    try:
        out = fn()
        _lib.check(lib.msam_profile_collect_family(n, ms, fl, by), "msam_profile_collect_family")
    finally:
        lib.msam_profile_enable(0)
    fams = [f for f in range(_lib.PROFILE_FAMILIES) for _ in range(n[f])]
    assert len(fams) <= 1, f"one call recorded {len(fams)} launches: {fams}"
    return out, (fams[0] if fams else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# generators

def _distinct(A, W):
    """Rows of A, rows of W and the k-columns of [A; W] are pairwise distinct."""
    a, w = A.float(), W.float()
    ok = torch.unique(w, dim=0).shape[0] == w.shape[0] and torch.unique(a, dim=0).shape[0] == a.shape[0]
    return ok and torch.unique(torch.cat([a, w], 0), dim=1).shape[1] == a.shape[1]


def exact_case(M, N, K, dt, seed, *, out_dtype=torch.float32, bias=True, table=None, table_rows=7, resid=None, resid_rows=0, relu=False,
               check_shares=True, dev=None):
    """Integer-valued operands (see the module docstring).  ``dt``: operand type (bf16 / fp16 / fp8 e4m3); ``table`` = table_cols or
    None; ``resid`` = None or the residual's torch dtype.  Returns a dict of CPU tensors plus 'ref' (the exact float64 result before the
    activation / output cast, [M, N], computed on ``dev``) - asserts the generator's conditions on it."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    assert _distinct(A, W), "exact_case: repeated rows / columns - choose another seed"
    c = dict(M=M, N=N, K=K, dt=dt, out_dtype=out_dtype, relu=relu, resid_rows=resid_rows)
    fp8 = dt == FP8_T
    amp = 4.0 if fp8 else 1.0
    if fp8:
        c["row_scale"] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (M,), generator=g)]      # powers of two: the scaled sums stay integers
        c["col_scale"] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (N,), generator=g)]
    c["A"], c["W"] = A.to(dt), W.to(dt)
    o16 = out_dtype if out_dtype in THRESH16 else (dt if dt in THRESH16 else torch.bfloat16)
    if bias:
        # |dot| <= 6 sigma = 6 * 4 sqrt(K) (sigma^2 = 16 per product; the assertion on min |ref| below holds the seed to it), table and
        # residual <= 600; the span keeps the type's spacing small enough (<= 32 mostly) for ties to stay frequent
        lo = THRESH16[o16] + int(amp * 24 * math.sqrt(K)) + 650
        mag = torch.randint(lo, lo + (2500 if o16 == torch.bfloat16 else 9000), (N,), generator=g)
        c["bias"] = (mag * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)).float()
    if table is not None:
        c["table"] = torch.randint(-100, 101, (table_rows, table), generator=g).float()
    if resid is not None:
        rng = 500 if resid == torch.float32 else 64          # exactly representable in the residual's type
        c["resid"] = torch.randint(-rng, rng + 1, (resid_rows or M, N), generator=g).float().to(resid)
    ref = preact64(c, dev)
    assert float(ref.abs().max()) < 2 ** 22 and bool((ref == ref.round()).all())
    if bias:
        assert float(ref.abs().min()) > THRESH16[o16], "exact_case: a result below the spacing-2 range"
    c["ref"] = ref
    if check_shares and bias and out_dtype in THRESH16:
        inexact, ties = shares(act64(ref, c).float(), out_dtype)
        assert inexact >= 0.25 and ties >= 0.01, f"exact_case: {inexact:.3f} inexact / {ties:.3f} ties in {out_dtype}"
    return c


def shares(v32, dt16):
    """(share of values that are inexact in ``dt16``, share that lie exactly half way between two ``dt16`` values); normal range."""
    low = bits(v32) & (0xFFFF if dt16 == torch.bfloat16 else 0x1FFF)
    half = 0x8000 if dt16 == torch.bfloat16 else 0x1000
    return float((low != 0).float().mean()), float((low == half).float().mean())


def random_case(M, N, K, dt, seed, *, bias=True, table=None, table_rows=7, resid=None, resid_rows=0, relu=False, scale=1.0,
                out_dtype=torch.float32, dev=None):
    """Gaussian operands as in tests/test_gpu_kernels.py: a ~ N(0, 1), w ~ N(0, 1 / K), fp32 bias / table / residual ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    c = dict(M=M, N=N, K=K, dt=dt, out_dtype=out_dtype, relu=relu, resid_rows=resid_rows)
    c["A"] = (torch.randn(M, K, generator=g) * scale).to(dt)
    c["W"] = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt)
    if dt == FP8_T:
        c["row_scale"] = torch.rand(M, generator=g) + 0.5
        c["col_scale"] = torch.rand(N, generator=g) + 0.5
    if bias:
        c["bias"] = torch.randn(N, generator=g)
    if table is not None:
        c["table"] = torch.randn(table_rows, table, generator=g)
    if resid is not None:
        c["resid"] = torch.randn(resid_rows or M, N, generator=g).to(resid)
    c["ref"] = preact64(c, dev)
    return c


def operands(c):
    """``call``'s operand keywords of a case."""
    kw = {k: c[k] for k in ("bias", "table", "resid", "row_scale", "col_scale") if k in c}
    kw["resid_rows"] = c.get("resid_rows", 0) if "resid" in c else 0
    if c.get("relu"):
        kw["act"] = ACT_RELU
    return kw


# ---------------------------------------------------------------------------------------------------------------------------------
# references

def preact64(c, dev=None, defect=None):
    """float64 A W^T (* scales) + bias + table + residual of a case - exact for the integer cases.  ``defect``: see ``expected``."""
    dev = dev or torch.device("cpu")
    A, W = c["A"].to(dev).float().double(), c["W"].to(dev).float().double()
    M, N, K = A.shape[0], W.shape[0], A.shape[1]
    if defect == "lda_as_k" and M > 1:                      # the rows of the PADDED buffer (lda = K + 8, zeros in the padding) taken at pitch K
        pad = torch.zeros(M, K + 8, dtype=A.dtype, device=dev)
        pad[:, :K] = A
        A = pad.reshape(-1)[:M * K].reshape(M, K)
    v = A @ W.t()
    if defect == "drop_ktile":
        v = v - A[:, K - 64:] @ W[:, K - 64:].t()
    elif defect == "dup_ktile":
        v = v + A[:, :64] @ W[:, :64].t()
    elif defect == "swap_aw_frag":                         # first 16 x 16 block, first k-step of 32: the two fragments exchanged
        m = min(M, 16)
        blk = A[:m, :32] @ W[:m, :32].t()
        v[:m, :m] += blk.t() - blk
    if "row_scale" in c:
        v = v * c["row_scale"].to(dev).double()[:, None] * c["col_scale"].to(dev).double()[None, :]
    if "bias" in c:
        v = v + c["bias"].to(dev).double()
    rows = torch.arange(M, device=dev)
    if "table" in c:
        t = c["table"].to(dev).double()
        tr = (rows + (1 if defect == "table_row_off" else 0)) % t.shape[0]
        v[:, :t.shape[1]] += t[tr]
        if defect == "table_col_le" and t.shape[1] < N:    # the four columns AT table_cols take the table too
            v[:, t.shape[1]:t.shape[1] + 4] += t[tr][:, -4:]
    if "resid" in c:
        r = c["resid"].to(dev).double()
        if c.get("resid_rows"):
            rr = rows.clamp(max=r.shape[0] - 1) if defect == "resid_nowrap" else rows % c["resid_rows"]
        else:
            rr = rows
        v = v + r[rr]
    if defect == "swap_rows" and M > 1:
        v[[0, 1]] = v[[1, 0]]
    return v


def act64(v, c):
    return v.clamp(min=0) if c.get("relu") else v


def rne16(v32, dt16, defect=None):
    """fp32 -> 16-bit, round to nearest even (torch's cast).  Defects: 'truncate' (towards zero), 'double_round' (through the OTHER type)."""
    assert v32.dtype == torch.float32
    if defect == "truncate":
        keep = -0x10000 if dt16 == torch.bfloat16 else -0x2000
        return (bits(v32) & keep).view(torch.float32).to(dt16)
    if defect == "double_round":
        other = torch.float16 if dt16 == torch.bfloat16 else torch.bfloat16
        return v32.to(other).float().to(dt16)
    return v32.to(dt16)


def split_qkv(v, tokens, heads, head_dim, defect=None):
    """[B tokens, 3 heads head_dim] -> q, k, v of [B, heads, tokens, head_dim]."""
    B = v.shape[0] // tokens
    if defect == "qkv_cross":
        return tuple(v.reshape(B, tokens, heads, 3, head_dim).permute(3, 0, 2, 1, 4).contiguous())
    return tuple(v.reshape(B, tokens, 3, heads, head_dim).permute(2, 0, 3, 1, 4).contiguous())


def split_kv(v, tokens, defect=None):
    """[B tokens, 256] -> k [B tokens, 128], vT [B, 128, tokens]."""
    B = v.shape[0] // tokens
    vv = v[:, 128:].reshape(B, tokens, 128)
    return v[:, :128].contiguous(), (vv.reshape(B, 128, tokens) if defect == "vt_untransposed" else vv.permute(0, 2, 1)).contiguous()


def hilo(v32, dt16, defect=None):
    """[hi | lo | hi] operand pairs of out_mode 3: hi = rne16(v), lo = rne16(v - hi)."""
    hi = rne16(v32, dt16, defect)
    lo = rne16(v32 - (v32 if defect == "lo_from_unrounded" else hi.float()), dt16)
    return torch.cat([lo, hi, hi] if defect == "hilo_swapped" else [hi, lo, hi], 1)


def expected(c, dev=None, out_mode=0, heads=0, head_dim=0, tokens=0, defect=None, v32=None):
    """The outputs of a launch of case ``c`` as a dict (out / q, k, v / k, v), from its exact reference - or from ``v32``, the fp32 output
    of a twin launch.  ``defect`` names a deliberate mistake (tests/test_gemm_routes_host.py lists them)."""
    od = c["out_dtype"]
    if v32 is None:
        v32 = act64(preact64(c, dev, defect), c).float()
    if out_mode == 3:
        return {"out": hilo(v32, od, defect)}
    o = v32 if od == torch.float32 else rne16(v32, od, defect)
    if out_mode == 1:
        return dict(zip(("q", "k", "v"), split_qkv(o, tokens, heads, head_dim, defect)))
    if out_mode == 2:
        return dict(zip(("k", "v"), split_kv(o, tokens, defect)))
    return {"out": o}


def assert_bits(got, exp, what):
    for nm, e in exp.items():
        g = got[nm] if isinstance(got, dict) else getattr(got, nm)
        e = e.to(g.device)
        if not same_bits(g, e):
            bad = (bits(g) != bits(e)).nonzero()
            first = tuple(int(x) for x in bad[0])
            raise AssertionError(f"{what}: output {nm}: {bad.shape[0]} of {g.numel()} elements differ; first at {first}: "
                                 f"got {float(g[first])!r}, expected {float(e[first])!r}")


def err_over_tol(got, ref64, atol, rtol):
    """max |got - ref| / (atol + rtol |ref|); inf if ``got`` is not finite."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref64).abs() / (atol + rtol * ref64.abs())).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm and GELU references

def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def layernorm64(pre, ln_w, ln_b, eps, mode):
    """float64 LayerNorm over the 256-wide row (mode 1) or over each group of 64 columns followed by the exact GELU (mode 2)."""
    M = pre.shape[0]
    x = pre.reshape(M, 1, 256) if mode == 1 else pre.reshape(M, 4, 64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps) * ln_w.double() + ln_b.double()
    return (gelu64(y) if mode == 2 else y).reshape(M, 256)


def gelu_constants():
    """The four constants of ``gelu_erf2`` as written in csrc/common.h."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "micro_sam_amd", "csrc", "common.h")).read()
    body = src[src.index("MSAM_DEVINL f32x2_t gelu_erf2(f32x2_t x)"):]
    body = body[:body.index("return r - t * e;")]
    cs = [float(x) for x in re.findall(r"(-\d+\.\d+)f", body)]
    assert len(cs) == 4, cs
    return cs


def gelu_formula64(x):
    """``gelu_erf2``'s formula in float64: max(x, 0) - |x| 2^q(|x|), q a cubic in |x|."""
    c3, c2, c1, c0 = gelu_constants()
    x = np.asarray(x, dtype=np.float64)
    t = np.abs(x)
    q = ((c3 * t + c2) * t + c1) * t + c0
    return np.maximum(x, 0.0) - t * np.exp2(q)


def gelu_design_error():
    """(max |formula - erf-GELU| on a dense grid over [-12, 12], the x where it occurs): the approximation's own error, arithmetic aside."""
    x = np.linspace(-12.0, 12.0, 2400001)
    exact = gelu64(torch.from_numpy(x)).numpy()
    d = np.abs(gelu_formula64(x) - exact)
    i = int(d.argmax())
    return float(d[i]), float(x[i])
