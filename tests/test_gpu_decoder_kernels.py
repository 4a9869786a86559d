"""The small kernels of csrc/decoder.hip on the device, one at a time, through the raw ABI: prompt encoding (``msam_prompt_encode``,
the token block of ``msam_decoder_prompt_prefix``, the dense grid of ``msam_decoder_prepare_const``), the token-side attention kernels
(``msam_dec_token_self_attention``, ``msam_dec_t2i_attention`` with group 0 / 4 / 8 / 16) and the source stream
(``msam_dec_source_stream``, ``msam_dec_tokens_from_sparse``, ``msam_dec_add_cast``) in the library's 16-bit type.

References, bounds, input families and the case table are tests/decoder_kernels_ref.py (read its docstring first): exact families bit
for bit, per-element float64 rounding bounds everywhere.  tests/test_decoder_kernels_host.py runs the table on the CPU and shows by
mutation that its assertions notice a wrong kernel.  Every output is a slice of a larger buffer between two guard zones of a fixed bit
pattern that must come back unchanged, is pre-filled with that pattern (a NaN in fp16, bf16 and fp32: an element that is not written
is seen), and every call is made twice and must return the same bits (no atomics).  The fp64 references of the attention and mask
cases are computed on the device.  The bf16 decoder build (MSAM_DEC_F16 = 0) is not covered (the host shim cannot build it either).

LARGEST err / bound (a ratio above 1 fails; the test prints the table), host emulation | MI355X:
  sparse rows 0.399 | 0.399      prompt tokens 0.399 | 0.399      dense pe 0.579 | 0.575      self attention 0.961 | 0.961
  t2i_attn 0.223 | 0.223         t2i_shared<4> 0.186 | 0.197      t2i_shared<8> 0.216 | 0.228  t2i_shared<16> 0.216 | 0.223
  mask dense, cubic / erf: dense weights 0.007 / 0.005 | 0.006 / 0.006, flat 0.155 / 0.086 | 0.155 / 0.086, small2 0.008 / 0.007 | 0.009 / 0.007
  mask keys, cubic / erf:  dense 0.931 / 0.926 | 0.931 / 0.926, flat 0.995 / 0.993 | 0.995 / 0.993, small2 0.942 / 0.927 | 0.942 / 0.927
(the 16-bit outputs sit near 1 because their last rounding alone is half an ulp of the bound; the host ran the reduced shared-kernel
table of its docstring).  The two GELU forms on randn * 4: 14.0 bounds apart on the flat weights, 1.3 on the dense ones, on both.
INTRINSICS in isolation on the MI355X, in ulp of the result (a-priori constant): sinf 1.342 (4), cosf 1.337 (4), erff 0.0 after the two
roundings around it (16), v_exp_f32 0.334 after the product's rounding (1).  ``__expf`` reaches 16-bit outputs only and is not isolated here.
No kernel defect was found: the tail-group merge at odd ``left`` and the fp16 subnormal probabilities of the rising family are within bounds.
"""
import math

import numpy as np
import pytest
import torch

import decoder_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _same_bits(a, b):
    if isinstance(a, tuple):
        return all(_same_bits(x, y) for x, y in zip(a, b))
    if a is None or isinstance(a, bool):
        return a == b
    return np.array_equal(R._bits(a), R._bits(b))


def _twice(name):
    fn = getattr(R.Backend, name)

    def call(self, *args, **kw):
        first, again = fn(self, *args, **kw), fn(self, *args, **kw)
        assert _same_bits(first, again), f"{name}: the second call returned other bits"
        return first
    return call


class DeviceBackend(R.Backend):
    """Device tensors behind the call layer; outputs between guard zones; every call twice."""
    where = "gpu"

    def __init__(self, dev):
        from micro_sam_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        self.dtype, self.stream = _lib.decoder_dtype(), _lib.stream_ptr()

    def last_error(self):
        return self.lib.msam_last_error().decode("utf-8", "replace")

    def sync(self):
        torch.cuda.synchronize()

    def _in(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.reshape(-1).view(np.uint8)).to(self.dev), 0

    def _in16(self, t):
        return t.contiguous().view(torch.int16).reshape(-1).to(self.dev), 0

    def _out(self, nbytes):
        assert nbytes % 2 == 0
        return torch.full((R.GUARD + nbytes // 2,), R.PATTERN16, dtype=torch.int16, device=self.dev), R.GUARD // 2

    def _scratch(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.dev), 0

    def _ptr(self, h):
        return h[0].data_ptr() + h[1] * h[0].element_size()

    def _read(self, h, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize // 2
        return h[0][h[1]:h[1] + n].cpu().numpy().view(dtype).reshape(shape).copy()

    def _guards_ok(self, h):
        g = R.GUARD // 2
        return bool((h[0][:g] == R.PATTERN16).all()) and bool((h[0][-g:] == R.PATTERN16).all())


for _name in ("prompt_encode", "prompt_tokens", "dense_pe", "self_attention", "t2i_attention", "source_stream", "tokens_from_sparse", "add_cast"):
    setattr(DeviceBackend, _name, _twice(_name))


@pytest.fixture(scope="module")
def gpu(dev):
    be = DeviceBackend(dev)
    if be.dtype != torch.float16:
        pytest.skip("the table's exact families are those of the fp16 decoder build")
    return be


@pytest.fixture(scope="module")
def w():
    return R.make_weights()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest err / bound on the device:\n" + R.format_ratios("gpu"))


def _assert(fails):
    assert not fails, "\n".join(f[2] for f in fails)


# ---- prompt encoding

@pytest.mark.parametrize("via", ["encode", "tokens"])
@pytest.mark.parametrize("Np,boxes", R.PROMPT_CASES)
def test_sparse_rows_and_prompt_tokens(gpu, w, Np, boxes, via):
    """Every coordinate and label of the table, the row order points -> padding -> corners; 10 points and a box are refused by a decode."""
    _assert(R.run_sparse_case(gpu, w, Np, boxes, via))


def test_dense_positional_encoding(gpu, w):
    _assert(R.run_dense_pe(gpu, w))


@pytest.fixture(scope="module")
def embedding():
    return np.random.default_rng(9).standard_normal((R.C, R.T)).astype(np.float32)


@pytest.mark.parametrize("tag", R.MASK_WEIGHT_SETS)
def test_mask_downscaling_in_both_gelu_forms_and_the_flag_acts(gpu, embedding, tag):
    """The seven masks in both GELU forms, dense and keys form; on the "flat" weights the two forms stand more than 10 bounds apart."""
    wm = R.mask_weights(tag)
    f0, cubic, b0 = R.run_masks(gpu, wm, 0, embedding, dev="cuda", tag=tag)
    f1, erf, b1 = R.run_masks(gpu, wm, 1, embedding, dev="cuda", tag=tag)
    _assert(f0 + f1)
    apart = float((np.abs(cubic[0].astype(np.float64) - erf[0]) / torch.maximum(b0[0], b1[0]).cpu().numpy()).max())
    print(f"\nthe two GELU forms on randn * 4, {tag} weights: {apart:.1f} bounds apart")
    assert tag != "flat" or apart > 10


# ---- source stream

def test_source_stream_is_exact(gpu, w):
    _assert(R.run_source_exact(gpu, w))


def test_tokens_from_sparse_copies(gpu, w):
    _assert(R.run_tokens_from_sparse(gpu, w))


def test_add_cast_is_exact(gpu):
    _assert(R.run_add_cast(gpu))


# ---- attention

@pytest.mark.parametrize("P", R.SELF_P)
@pytest.mark.parametrize("Nt", R.SELF_NT)
def test_self_attention_table(gpu, P, Nt):
    _assert(R.run_self_attention(gpu, P, Nt, dev="cuda"))


@pytest.mark.parametrize("kv_shared", [0, 1])
@pytest.mark.parametrize("P", R.T2I_P)
@pytest.mark.parametrize("Nt", R.T2I_NT)
def test_t2i_attention_table(gpu, Nt, P, kv_shared):
    """t2i_attn_kernel: 9 .. 16 tokens per prompt, shared (layer 0) and per-prompt (behind a mask prompt) K / V^T."""
    _assert(R.run_t2i(gpu, 0, P, Nt, kv_shared, dev="cuda"))


@pytest.mark.parametrize("slot", range(5))
@pytest.mark.parametrize("Nt", R.SHARED_NT)
@pytest.mark.parametrize("G", R.SHARED_G)
def test_t2i_shared_table(gpu, G, Nt, slot):
    """t2i_shared_kernel<G> at P = 1, G - 1, G, G + 1, 2 G + 1 (slot 0 .. 4): every family, and the same prompts in a launch of P - 1."""
    _assert(R.run_t2i(gpu, G, R.shared_p(G)[slot], Nt, 1, dev="cuda"))


# ---- the intrinsics on their own

def test_intrinsics_are_within_the_constant_the_bounds_use(gpu, w):
    """sinf, cosf, erff and v_exp_f32 where a float64 value isolates them (decoder_kernels_ref.measure_intrinsics); ``__expf`` reaches
    16-bit outputs only.  Prints the measured constants in ulp of the result; one above its a-priori constant fails."""
    m = R.measure_intrinsics(gpu, w)
    e_sin, e_cos, e_erf, e_exp2 = m["sinf"], m["cosf"], m["erff"], m["v_exp_f32"]
    print(f"\nmeasured on the device, in ulp of the result: sinf {e_sin:.3f}, cosf {e_cos:.3f} (bounds use {R.E_SINCOS}); erff {e_erf:.3f} (after the "
          f"roundings around it; bounds use {R.E_ERF}); v_exp_f32 {e_exp2:.3f} (after the product's rounding; bounds use {R.E_EXP2})")
    assert e_sin <= R.E_SINCOS and e_cos <= R.E_SINCOS and e_erf <= R.E_ERF and e_exp2 <= R.E_EXP2


def test_refusals_leave_the_outputs_alone(gpu, w):
    """Every new entry: 1, an error text that names the entry, nothing written."""
    bad = R.run_refusals(gpu, w)
    assert not bad, "\n".join(bad)
