"""The split16 kernels' C ABI calls on the operand dicts of tests/split16_ref.py, shared by the host test (the host build of
csrc/strict.hip, CPU tensors, stream None) and the device test (libmsam_hip.so, CUDA tensors).  Every output is pre-filled with NaN;
workspaces are sized EXACTLY to the documented byte count and followed by a NaN guard region that must stay untouched."""
import ctypes as C

import torch

import split16_ref as R

GUARD = 4096                                          # floats behind an exactly sized workspace


def _p(t):
    return None if t is None else t.data_ptr()


def _check(lib, status, what):
    assert status == 0, (what, status, lib.msam_last_error())


def gemm(lib, L, inp, split=True, stream=None):
    """msam_strict_gemm on a make_product dict -> out fp32 ([M, N]; [4 M, N / 4] for the 2 x 2 store)."""
    a, w = inp["a"], inp["w"]
    N, K = w.shape
    conv, shuf = inp.get("conv"), inp.get("shuffle")
    M = a.shape[0]
    out = torch.full((4 * M, N // 4) if shuf else (M, N), float("nan"), dtype=torch.float32, device=a.device)
    p = L.SGemmParams()
    p.A, p.lda, p.W, p.ldw, p.M, p.N, p.K = a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), M, N, K
    if inp.get("a2") is not None:
        p.A2, p.lda2, p.a2_rows, p.a2_cols = inp["a2"].data_ptr(), inp["a2"].stride(0), int(inp["a2_rows"]), int(inp.get("a2_cols") or 0)
    p.bias, p.act = _p(inp.get("bias")), int(inp.get("act") or 0)
    if inp.get("res") is not None:
        p.res, p.ldr, p.res_rows = inp["res"].data_ptr(), inp["res"].stride(0), int(inp["res_rows"])
    p.col_scale, p.col_shift = _p(inp.get("col_scale")), _p(inp.get("col_shift"))
    if conv:
        p.conv_h, p.conv_w, p.conv_c = conv[1], conv[2], conv[3]
    if shuf:
        p.shuffle_h, p.shuffle_w, p.shuffle_c = shuf[1], shuf[2], shuf[3]
    p.out, p.ldc = out.data_ptr(), out.stride(0)
    if split:
        p.split16, p.a_scale, p.w_scale = 1, 1.0, float(inp["w_scale"])
    _check(lib, lib.msam_strict_gemm(C.byref(p), stream), "msam_strict_gemm")
    return out


def prepare_pairs(lib, w, scale, permute, stream=None):
    """msam_split16_prepare_pairs -> fp16 [N, 2 K] behind which a guard of NaN halves must stay untouched."""
    N, K = w.shape
    buf = torch.full((N * 2 * K + GUARD,), float("nan"), dtype=torch.float16, device=w.device)
    _check(lib, lib.msam_split16_prepare_pairs(w.data_ptr(), N, K, float(scale), int(permute), buf.data_ptr(), stream), "prepare_pairs")
    return buf[:N * 2 * K].reshape(N, 2 * K), buf[N * 2 * K:]


def _workspace(nbytes, dev):
    """An exactly sized workspace (zeros) followed by the NaN guard; -> (whole buffer, guard view)."""
    assert nbytes % 4 == 0
    buf = torch.zeros(nbytes // 4 + GUARD, dtype=torch.float32, device=dev)
    buf[nbytes // 4:] = float("nan")
    return buf, buf[nbytes // 4:]


def guard_untouched(guard):
    return bool(torch.isnan(guard).all())


def t2i(lib, L, inp, ldq=128, ldo=128, stream=None):
    """msam_split16_t2i_attention on a make_t2i dict -> (out fp32 [B, Tk, 128], workspace guard)."""
    B, Tk = inp["q"].shape[:2]
    dev = inp["q"].device
    q = torch.full((B * Tk, ldq), float("nan"), dtype=torch.float32, device=dev)
    q[:, :128] = inp["q"].reshape(B * Tk, 128)
    out = torch.full((B * Tk, ldo), float("nan"), dtype=torch.float32, device=dev)
    ws, guard = _workspace(B * 131072, dev)
    p = L.ST2IParams()
    p.keys, p.key_batch_stride, p.pos, p.q, p.ldq = inp["keys"].data_ptr(), R.T * R.C, inp["pos"].data_ptr(), q.data_ptr(), ldq
    p.wk, p.wv, p.bv, p.denom = inp["wk"].data_ptr(), inp["wv"].data_ptr(), inp["bv"].data_ptr(), float(inp["denom"])
    p.out, p.ldo, p.B, p.Tk = out.data_ptr(), ldo, B, Tk
    p.workspace, p.workspace_bytes = ws.data_ptr(), B * 131072
    _check(lib, lib.msam_split16_t2i_attention(C.byref(p), stream), "msam_split16_t2i_attention")
    if ldo > 128:
        assert bool(torch.isnan(out[:, 128:]).all()), "t2i wrote behind the 128 channels of an output row"
    return out[:, :128].reshape(B, Tk, 128), guard


def _i2t_params(L, inp, out):
    B, Tk = inp["tok_k"].shape[:2]
    p = L.SI2TParams()
    p.keys, p.key_batch_stride, p.pos = inp["keys"].data_ptr(), (0 if inp["shared"] else R.T * R.C), inp["pos"].data_ptr()
    p.wq, p.bq, p.wo, p.bo = inp["wq"].data_ptr(), inp["bq"].data_ptr(), inp["wo"].data_ptr(), inp["bo"].data_ptr()
    p.tok_k, p.tok_v, p.ld_tok, p.tok_batch_stride = inp["tok_k"].data_ptr(), inp["tok_v"].data_ptr(), 128, Tk * 128
    p.ln_weight, p.ln_bias, p.ln_eps, p.denom = inp["ln_w"].data_ptr(), inp["ln_b"].data_ptr(), float(inp["ln_eps"]), float(inp["denom"])
    p.out, p.B, p.Tk = out.data_ptr(), B, Tk
    return p


def _i2t_out(inp, in_place):
    B = inp["tok_k"].shape[0]
    if in_place:
        assert not inp["shared"]
        return inp["keys"]
    return torch.full((B, R.T, R.C), float("nan"), dtype=torch.float32, device=inp["keys"].device)


def i2t_folded(lib, L, inp, in_place=False, stream=None):
    """msam_split16_i2t_block -> (out fp32 [B, 4096, 256], workspace guard); ``in_place``: out = keys (pass a dict with cloned keys)."""
    B = inp["tok_k"].shape[0]
    out = _i2t_out(inp, in_place)
    ws, guard = _workspace(B * 131328, out.device)
    p = _i2t_params(L, inp, out)
    _check(lib, lib.msam_split16_i2t_block(C.byref(p), ws.data_ptr(), B * 131328, stream), "msam_split16_i2t_block")
    return out, guard


def i2t_unfolded(lib, L, inp, pairs=None, in_place=False, stream=None):
    """msam_strict_i2t_block with split16 = 1; ``pairs`` = (wq pairs, wo pairs permuted) of prepare_pairs with the dict's scales."""
    out = _i2t_out(inp, in_place)
    p = _i2t_params(L, inp, out)
    p.split16, p.wq_scale, p.wo_scale = 1, float(inp["wq_scale"]), float(inp["wo_scale"])
    if pairs is not None:
        p.wq_pairs, p.wo_pairs = pairs[0].data_ptr(), pairs[1].data_ptr()
    _check(lib, lib.msam_strict_i2t_block(C.byref(p), stream), "msam_strict_i2t_block")
    return out


class tuned:
    """Context: msam_tune_set knobs, restored to the library's defaults on exit."""
    DEFAULTS = {"sgemm_bufs": 1, "sgemm_small_below": 512}

    def __init__(self, lib, **knobs):
        self.lib, self.knobs = lib, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            assert k in self.DEFAULTS and self.lib.msam_tune_set(k.encode(), int(v)) == 0, k
        return self

    def __exit__(self, *exc):
        for k in self.knobs:
            assert self.lib.msam_tune_set(k.encode(), self.DEFAULTS[k]) == 0
        return False


ROUTES = {"tile64": {"sgemm_small_below": 1 << 30}, "tile128_nbuf1": {"sgemm_small_below": 0, "sgemm_bufs": 1},
          "tile128_nbuf2": {"sgemm_small_below": 0, "sgemm_bufs": 2}}


def ratio(got, ref, bound):
    """max |got - ref| / bound over EVERY element (inf where a bound of 0 is missed, NaN-safe: a NaN output gives inf)."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def up2(lib, L, inp, stream=None):
    """msam_strict_upscale2 on a make_up2 dict -> (low_res fp32 [P, nmask, 256, 256], guard behind it)."""
    P, nmask = int(inp["P"]), int(inp["nmask"])
    n = P * nmask * 65536
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=inp["u1"].device)
    q = L.SUp2Params()
    q.u1, q.ln_weight, q.ln_bias, q.ln_eps = inp["u1"].data_ptr(), inp["ln_w"].data_ptr(), inp["ln_b"].data_ptr(), float(inp["ln_eps"])
    q.w2, q.b2, q.w_scale = inp["w2"].data_ptr(), inp["b2"].data_ptr(), float(inp["w_scale"])
    q.hyper, q.hyper_ld, q.mask0, q.nmask, q.low_res, q.P = inp["hyper"].data_ptr(), int(inp["hyper_ld"]), int(inp["mask0"]), nmask, buf.data_ptr(), P
    _check(lib, lib.msam_strict_upscale2(C.byref(q), stream), "msam_strict_upscale2")
    return buf[:n].reshape(P, nmask, 256, 256), buf[n:]


def relpos(lib, inp, stream=None):
    """msam_split16_relpos_attention on a make_relpos dict -> (out fp32 [B G G, heads hd], guard behind it)."""
    B, heads, hd, G = inp["B"], inp["heads"], inp["hd"], inp["G"]
    n = B * G * G * heads * hd
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=inp["qkv"].device)
    _check(lib, lib.msam_split16_relpos_attention(inp["qkv"].data_ptr(), inp["bqkv"].data_ptr(), inp["rel_h"].data_ptr(), inp["rel_w"].data_ptr(),
                                                  B, heads, hd, G, inp["window"], float(inp["scale"]), buf.data_ptr(), stream), "relpos")
    return buf[:n].reshape(B * G * G, heads * hd), buf[n:]
