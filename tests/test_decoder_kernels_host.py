"""The small kernels of csrc/decoder.hip on the CPU: the library compiled for the host (tests/hip_host_shim.build_library) and called
through its C ABI - ``msam_prompt_encode``, ``msam_decoder_prompt_prefix``, ``msam_decoder_prepare_const`` and the kernel-level entries
``msam_dec_*`` - on the case table, the exact families and the float64 rounding bounds of tests/decoder_kernels_ref.py (read its
docstring first).  This shows that the references and the bounds hold for a correct implementation before a GPU is involved;
tests/test_gpu_decoder_kernels.py runs the same table there.

THE MUTATION CHECK patches copies of decoder.hip (host only - nothing mutated is ever built for or run on a device), one defect each,
builds each copy alone with ``build_library(files=...)`` from a scratch source tree (the rest of the library as stubs that return 0:
the kernels under test need none of it) and requires that an assertion of the table reports the defect, exactly or by at least 4 bounds.
All mutations keep their accesses inside the guarded buffers of the call layer.  What the mutation check added to the families: the
one-hot family's values are non-zero and the second one-hot variant puts targets on the edges of the 32-key steps (a loop one step
short survives hashed targets with probability 31 / 32 per query); ``nt`` taken as ``NT`` in a tail group of ``t2i_shared_kernel`` is
NOT a defect - the merge loop's body is guarded by ``p < P``, the extra tiles do nothing - so the table carries its converse (the odd
tail's last tile dropped) instead.

The 16-bit type is fp16, the library's default.  The shim defines the decoder's type helpers for fp16 only, so the bf16 build
(MSAM_DEC_F16 = 0) is not covered here or on the device.

On the host the three group sizes of ``t2i_shared_kernel`` run every P of the table at Nt = 5 and 8 with the uniform, both one-hot and
the rising families (time: a launch of 33 prompts is 136 emulated workgroups); G = 4, the default, also runs Nt = 7 and every family."""
import ctypes
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import decoder_kernels_ref as R
import hip_host_shim as shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("msam_prompt_encode", "msam_decoder_prompt_prefix", "msam_decoder_prompt_prefix_bytes", "msam_decoder_workspace_bytes",
           "msam_decoder_const_bytes", "msam_decoder_prepare_const", "msam_decoder_dtype", "msam_dec_token_self_attention", "msam_dec_t2i_attention",
           "msam_dec_source_stream", "msam_dec_tokens_from_sparse", "msam_dec_add_cast")
PATTERN_IN = 0x3C00                                   # inputs' guard zones: 1.0 (a mutant that reads past a row reads a number)


class HostBackend(R.Backend):
    where, dtype, stream = "host", torch.float16, None

    def __init__(self, lib, error_fn="msam_last_error", where="host"):
        from micro_sam_amd import _lib
        self.lib, self.where = lib, where
        for name in ENTRIES:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _lib._PROTOS[name]
        self._err = getattr(lib, error_fn)
        self._err.restype = ctypes.c_char_p
        assert lib.msam_decoder_dtype() == _lib.F16

    def last_error(self):
        return (self._err() or b"").decode()

    def _buf(self, nbytes, pattern):
        assert nbytes % 2 == 0
        return np.full(2 * (R.GUARD // 2) + nbytes // 2, pattern, np.uint16)

    def _in(self, a):
        a = np.ascontiguousarray(a)
        buf = self._buf(a.nbytes, PATTERN_IN)
        buf.view(np.uint8)[R.GUARD:R.GUARD + a.nbytes] = a.reshape(-1).view(np.uint8)
        return buf, a.nbytes

    def _out(self, nbytes):
        return self._buf(nbytes, R.PATTERN16), nbytes

    def _scratch(self, nbytes):
        return np.zeros(nbytes + 2 * R.GUARD, np.uint8), nbytes

    def _ptr(self, h):
        return h[0].ctypes.data + R.GUARD

    def _read(self, h, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return h[0].view(np.uint8)[R.GUARD:R.GUARD + n].copy().view(dtype).reshape(shape)

    def _guards_ok(self, h):
        g = R.GUARD // 2
        return bool((h[0][:g] == R.PATTERN16).all() and (h[0][-g:] == R.PATTERN16).all())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostBackend(shim.build_library(str(tmp_path_factory.mktemp("host_dec_kernels")), ROOT))


@pytest.fixture(scope="module")
def w():
    return R.make_weights()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest err / bound on the host:\n" + R.format_ratios("host"))


def _assert(fails):
    assert not fails, "\n".join(f[2] for f in fails)


# ---- prompt encoding

@pytest.mark.parametrize("via", ["encode", "tokens"])
@pytest.mark.parametrize("Np,boxes", R.PROMPT_CASES)
def test_sparse_rows_and_prompt_tokens(host, w, Np, boxes, via):
    _assert(R.run_sparse_case(host, w, Np, boxes, via))


def test_dense_positional_encoding(host, w):
    _assert(R.run_dense_pe(host, w))


@pytest.fixture(scope="module")
def embedding():
    return np.random.default_rng(9).standard_normal((R.C, R.T)).astype(np.float32)


@pytest.mark.parametrize("tag", R.MASK_WEIGHT_SETS)
def test_mask_downscaling_in_both_gelu_forms_and_the_flag_acts(host, embedding, tag):
    wm = R.mask_weights(tag)
    f0, cubic, b0 = R.run_masks(host, wm, 0, embedding, tag=tag)
    f1, erf, b1 = R.run_masks(host, wm, 1, embedding, tag=tag)
    _assert(f0 + f1)
    apart = float((np.abs(cubic[0].astype(np.float64) - erf[0]) / torch.maximum(b0[0], b1[0]).numpy()).max())
    print(f"\nthe two GELU forms on randn * 4, {tag} weights: {apart:.1f} bounds apart")
    assert tag != "flat" or apart > 10


# ---- source stream

def test_source_stream_is_exact(host, w):
    _assert(R.run_source_exact(host, w))


def test_tokens_from_sparse_copies(host, w):
    _assert(R.run_tokens_from_sparse(host, w))


def test_add_cast_is_exact(host):
    _assert(R.run_add_cast(host))


# ---- attention

@pytest.mark.parametrize("P", R.SELF_P)
@pytest.mark.parametrize("Nt", R.SELF_NT)
def test_self_attention_table(host, P, Nt):
    _assert(R.run_self_attention(host, P, Nt))


@pytest.mark.parametrize("kv_shared", [0, 1])
@pytest.mark.parametrize("P", R.T2I_P)
@pytest.mark.parametrize("Nt", R.T2I_NT)
def test_t2i_attention_table(host, Nt, P, kv_shared):
    _assert(R.run_t2i(host, 0, P, Nt, kv_shared))


HOST_SHARED = [(G, Nt, R.T2I_FAMILIES if (G == 4) else ("uniform", "onehot:0", "onehot:1", "rising"))
               for G in R.SHARED_G for Nt in (R.SHARED_NT if G == 4 else (5, 8))]


@pytest.mark.parametrize("G,Nt,families", HOST_SHARED, ids=lambda v: str(v) if isinstance(v, int) else str(len(v)))
def test_t2i_shared_table(host, G, Nt, families):
    fails = []
    for P in R.shared_p(G):
        fails += R.run_t2i(host, G, P, Nt, 1, families=families)
    _assert(fails)


def test_the_table_covers_what_the_issue_names():
    assert R.SELF_NT == (1, 5, 7, 8, 9, 15, 16) and R.T2I_NT == (9, 12, 16) and R.SHARED_NT == (5, 7, 8) and R.SHARED_G == (4, 8, 16)
    assert all(R.shared_p(G) == (1, G - 1, G, G + 1, 2 * G + 1) for G in R.SHARED_G)
    assert {n for n, _ in R.PROMPT_CASES} == {0, 1, 2, 10} and len(R.PROMPT_CASES) == 7
    labels, coords = set(), set()
    for Np, boxes in R.PROMPT_CASES:
        pts, lab, bx = R.prompt_inputs(Np, boxes)
        if Np:
            labels |= set(lab.reshape(-1).tolist())
            coords |= {tuple(p) for p in pts.reshape(-1, 2).tolist()}
    assert labels == set(R.LABELS) and {tuple(map(float, np.float32(p))) for p in R.POINTS} <= coords
    for P, Nt in ((33, 8), (3, 16)):
        pi = R.onehot_target(P, Nt, 0)
        assert pi.unique().numel() == pi.numel()
    assert set(R.onehot_target(3, 8, 1).reshape(-1).tolist()) == set(R.EDGE_KEYS)
    m = R.make_masks()[R.MASK_KINDS.index("distinct")]
    assert len({tuple(r) for r in m.tolist()}) == 256 and len({tuple(r) for r in m.T.tolist()}) == 256


def test_refusals_leave_the_outputs_alone(host, w):
    bad = R.run_refusals(host, w)
    assert not bad, "\n".join(bad)


# ---- the mutation check

STUBS = "\n".join(
    ['extern "C" long msam_chain_const2_bytes() { return 128L * 128 * 4 + 4 * 512 + 128L * 256 * 2; }'] +
    [f'extern "C" long {n}() {{ return 0; }}' for n in ("msam_chain_handover_bytes", "msam_chain_tables2_bytes", "msam_chain_tables_bytes", "msam_i2t_fold_operand_bytes")] +
    [f'extern "C" int {n}() {{ return 0; }}' for n in (
        "msam_cast_f32_split16", "msam_chain_prepare_const2", "msam_chain_prepare_tables", "msam_chain_prepare_tables2_c", "msam_decoder_image_layer",
        "msam_gemm_bf16", "msam_gemm_group_bf16", "msam_i2t01_fused", "msam_i2t01_fused_handover", "msam_i2t0_t2i_fused", "msam_i2t0_t2i_fused_v2",
        "msam_i2t0_t2i_fused_v2_handover", "msam_i2t_fold_layer", "msam_i2t_fold_operands", "msam_i2t_fold_operands_values", "msam_layernorm",
        "msam_t2i_fold_attention", "msam_upscale_fused_range", "msam_wsgemm_bf16")] +
    ["int g_tune_chain_handover = 0, g_tune_chain_variant = 0, g_tune_dec_chain = 0, g_tune_dec_chain_min_p = 0;"]) + "\n"


def _sub(old, new, count=1):
    def apply(src):
        assert src.count(old) == count, (old, src.count(old), count)
        return src.replace(old, new)
    return apply


_PE_CALL = "pe_encode(G, px / 1024.f, py / 1024.f, j, s, co);"
_SPARSE = lambda be, w: [f for Np, b in R.PROMPT_CASES for via in ("encode", "tokens") for f in R.run_sparse_case(be, w, Np, b, via)]
_DENSE = lambda be, w: R.run_dense_pe(be, w)
_WSETS = [(t, R.mask_weights(t)) for t in R.MASK_WEIGHT_SETS]
_MASK0 = lambda be, w: [f for t, wm in _WSETS for f in R.run_masks(be, wm, 0, tag=t)[0]]
_MASK1 = lambda be, w: [f for t, wm in _WSETS for f in R.run_masks(be, wm, 1, tag=t)[0]]
_MASKK = lambda be, w: R.run_masks(be, w, 0, np.random.default_rng(9).standard_normal((R.C, R.T)).astype(np.float32))[0]
_SELF = lambda be, w: [f for Nt in (5, 16) for f in R.run_self_attention(be, 3, Nt)]
_T2I = lambda be, w: R.run_t2i(be, 0, 3, 9, 0) + R.run_t2i(be, 0, 3, 9, 1)
_SHARED = lambda be, w: [f for P in (3, 5) for Nt in (5, 8) for f in R.run_t2i(be, 4, P, Nt, 1, families=("uniform", "onehot:0", "onehot:1", "rising"))]
_BOTH = lambda be, w: _T2I(be, w) + _SHARED(be, w)
# name -> (source edits, the part of the table that must report it)
MUTATIONS = {
    "G's two rows swapped": ([_sub("(x * G[j] + y * G[128 + j])", "(x * G[128 + j] + y * G[j])")], _SPARSE),
    "+0.5 missing": ([_sub(" * 2] + 0.5f, py = points[((long)p * Np + i) * 2 + 1] + 0.5f;", " * 2], py = points[((long)p * Np + i) * 2 + 1];", 2)], _SPARSE),
    "+0.5 missing at the box corners": ([_sub("+ 2 * k] + 0.5f, by = boxes[(long)p * 4 + 2 * k + 1] + 0.5f;", "+ 2 * k], by = boxes[(long)p * 4 + 2 * k + 1];", 2)], _SPARSE),
    "/1023 for /1024": ([_sub(_PE_CALL, _PE_CALL.replace("1024.f", "1023.f"), 2)], _SPARSE),
    "sine and cosine halves swapped": ([_sub("float v = c < 128 ? s : co;", "float v = c < 128 ? co : s;", 2)], _SPARSE),
    "2c-1 missing": ([_sub("const float x = 2.f * cx - 1.f, y = 2.f * cy - 1.f;", "const float x = cx, y = cy;")], _SPARSE),
    "label-0 and label-1 embeddings swapped": ([_sub("else if (lab == 0) v += point_embed[0 * C + c];", "else if (lab == 0) v += point_embed[1 * C + c];", 2),
                                                _sub("else if (lab == 1) v += point_embed[1 * C + c];", "else if (lab == 1) v += point_embed[0 * C + c];", 2)], _SPARSE),
    "box-corner embeddings 2 and 3 swapped": ([_sub("point_embed[(2 + k) * C + c]", "point_embed[(3 - k) * C + c]", 2)], _SPARSE),
    "label -1 added to the Fourier row": ([_sub("if (lab == -1) v = not_a_point[c];", "if (lab == -1) v += not_a_point[c];", 2)], _SPARSE),
    "a padding row although a box is present": ([_sub("if (Np > 0 && !boxes) { tp[row * C + c] = not_a_point[c]; ++row; }", "if (Np > 0) { tp[row * C + c] = not_a_point[c]; ++row; }", 2)], _SPARSE),
    "tx / ty swapped in the dense grid": ([_sub("const int ty = t >> 6, tx = t & 63;", "const int tx = t >> 6, ty = t & 63;")], _DENSE),
    "conv-1 taps transposed": ([_sub("mp.c1_w[ch * 4 + ky * 2 + kx]", "mp.c1_w[ch * 4 + kx * 2 + ky]")], _MASK0),
    "conv-2 h1[ky][kx] swapped": ([_sub("h1[ky][kx][ci]", "h1[kx][ky][ci]")], _MASK0),
    "LayerNorm divisor 1/3 for 1/4": ([_sub("var * 0.25f + 1e-6f", "var * (1.f / 3.f) + 1e-6f")], _MASK0),
    "1e-5 for 1e-6": ([_sub("var * 0.25f + 1e-6f", "var * 0.25f + 1e-5f")], _MASK0),
    "1e-5 for 1e-6 in the second norm": ([_sub("var * (1.f / 16.f) + 1e-6f", "var * (1.f / 16.f) + 1e-5f")], _MASK0),
    "exact_gelu ignored": ([_sub("mp.exact_gelu ? gelu_exact_f(z_) : gelu_erf(z_)", "gelu_erf(z_)", 2)], _MASK1),
    "the dense form's base with no_mask subtracted": ([_sub("const float base = dense_out ? mp.c3_b[c] : mp.c3_b[c] - no_mask[c];", "const float base = mp.c3_b[c] - no_mask[c];")], _MASK0),
    "the keys form's base without no_mask": ([_sub("const float base = dense_out ? mp.c3_b[c] : mp.c3_b[c] - no_mask[c];", "const float base = mp.c3_b[c];")], _MASKK),
    "wrong 4 ty row offset": ([_sub("(long)(4 * ty) * 256 + 4 * tx", "(long)(4 * tx) * 256 + 4 * ty")], _MASK0),
    "self-attention scale 1/sqrt(16)": ([_sub("acc *= 0.17677669529663687f;", "acc *= 0.25f;")], _SELF),
    "self-attention's padded j unmasked": ([_sub("} else acc = NEG_BIG;", "}")], _SELF),
    "alpha dropped": ([_sub("l = l * alpha + ps;", "l = l + ps;"), _sub("l[n] = l[n] * alpha + ps;", "l[n] = l[n] + ps;"),
                       _sub("o[0] *= alpha; o[1] *= alpha; o[2] *= alpha; o[3] *= alpha;", ""),
                       _sub("o[n][0] *= alpha; o[n][1] *= alpha; o[n][2] *= alpha; o[n][3] *= alpha;", "")], _BOTH),
    "the wave merge without its exponential": ([_sub("const float a = __expf(red[w][fr][0] - mm);", "const float a = 1.f;"),
                                                _sub("const float a = __expf(red[w][c][0] - mm);", "const float a = 1.f;")], _BOTH),
    "the key loop one step short": ([_sub("for (int t0 = t_begin; t0 < t_end; t0 += 32) {", "for (int t0 = t_begin; t0 < t_end - 32; t0 += 32) {", 2)], _BOTH),
    "kv_shared ignored": ([_sub("const int pk = kv_shared ? 0 : p;", "const int pk = 0;")], _T2I),
    "the fr >> 3 prompt mapping off by one": ([_sub("const int p = pg * G + n * 2 + (fr >> 3);\n        qf[n]", "const int p = pg * G + n * 2 + 1 - (fr >> 3);\n        qf[n]")], _SHARED),
    "tk < Nt dropped from the write guard": ([_sub("if (tk < Nt && p < P) {\n            const float mm", "if (p < P) {\n            const float mm")], _SHARED),
    "the odd tail's last tile not merged": ([_sub("const int nt = left >= G ? NT : (left + 1) >> 1;", "const int nt = left >= G ? NT : left >> 1;")], _SHARED),
}


def _source_tree(tmp, source):
    """A scratch copy of what build_library reads: csrc headers, the public header, the patched decoder.hip and the stubs."""
    csrc = os.path.join(tmp, "micro_sam_amd", "csrc")
    os.makedirs(csrc)
    os.makedirs(os.path.join(tmp, "include"))
    real = os.path.join(ROOT, "micro_sam_amd", "csrc")
    for n in os.listdir(real):
        if n.endswith(".h"):
            shutil.copy(os.path.join(real, n), csrc)
    shutil.copy(os.path.join(ROOT, "include", "msam_hip.h"), os.path.join(tmp, "include"))
    with open(os.path.join(csrc, "decoder.hip"), "w") as fh:
        fh.write(source)
    with open(os.path.join(csrc, "rest_stubs.hip"), "w") as fh:
        fh.write(STUBS)
    return tmp


def _build_alone(tmp_path_factory, source):
    tree = _source_tree(str(tmp_path_factory.mktemp("dec_tree")), source)
    lib = shim.build_library(str(tmp_path_factory.mktemp("dec_alone")), tree, files=["decoder.hip", "rest_stubs.hip"])
    return HostBackend(lib, "emu_last_error", "mutant")


@pytest.fixture(scope="module")
def mutants(tmp_path_factory):
    base = open(os.path.join(ROOT, "micro_sam_amd", "csrc", "decoder.hip")).read()

    def build(item):
        name, (edits, _) = item
        src = base
        for e in edits:
            src = e(src)
        assert src != base
        return name, _build_alone(tmp_path_factory, src)

    with ThreadPoolExecutor(8) as ex:
        return dict(ex.map(build, MUTATIONS.items()))


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_is_reported(mutants, w, name):
    """An exact assertion, a written guard zone, or a bound missed by a factor of 4 or more."""
    try:
        fails = MUTATIONS[name][1](mutants[name], w)
    except AssertionError as e:                        # the call layer's own assertions: a guard zone was written, output tokens not copied
        fails = [("exact", "call layer", str(e), float("inf"))]
    hits = [f for f in fails if f[0] == "exact" or f[3] >= 4.0]
    assert hits, f"'{name}' survives the table: it is missing a case"
    print(f"\n{name}: {hits[0][2]}")


def test_the_unmutated_source_alone_passes_what_the_mutants_run(tmp_path_factory, w):
    """The decoder file on its own with the stubs is a faithful stand for the library: the unpatched source passes the same runs."""
    be = _build_alone(tmp_path_factory, open(os.path.join(ROOT, "micro_sam_amd", "csrc", "decoder.hip")).read())
    _assert(R.run_sparse_case(be, w, 2, True, "tokens") + _DENSE(be, w) + _SELF(be, w) + R.run_t2i(be, 4, 5, 8, 1, families=("onehot:1", "rising")))
