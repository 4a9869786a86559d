"""Fine-tuning's attention kernels (csrc/train.hip) on the CPU: the whole file compiled for the host (tests/hip_host_shim.py), called
through its C ABI (``msam_attention_forward`` / ``_backward``, ``msam_relpos_attention_forward`` / ``_backward``: the launchers' route
conditions included) and held to the case table, the exact assertions and the float64 rounding bounds of
tests/train_attention_ref.py.  This shows that the reference and the bounds hold for a correct implementation before a GPU is involved
(tests/test_gpu_train_attention.py runs the same table there).

THE MUTATION CHECK builds nine mutated copies of the source (host only - nothing mutated is ever built for or run on a device) and
requires, for every mutation and every kernel form it touches, that an EXACT assertion of the table reports it: a table that a wrong
kernel passes is missing a case.  All mutations keep their accesses inside the buffers (the inputs here carry guard zones too: the
swapped j / Gw, j % Gw reads a few elements past a bias row).

The host run leaves out the ``peaked:first`` and ``peaked:random`` orders of the bounded families (time); every exact case runs."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hip_host_shim as shim
import train_attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                            # floats before and after every array
PATTERN = np.uint32(0x7FA5C3E1)                        # outputs: a NaN, so that an unwritten element is not finite
PATTERN_IN = np.uint32(0x3F9D70A4)                     # inputs: 1.23 (a mutant that reads past a row reads a number)
_VP, _I, _F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
ABI = {"msam_attention_forward": [_VP] * 3 + [_I] * 4 + [_F] + [_VP] * 3,
       "msam_attention_backward": [_VP] * 6 + [_I] * 4 + [_F] + [_VP] * 5,
       "msam_relpos_attention_forward": [_VP] * 5 + [_I] * 4 + [_F] + [_VP] * 3,
       "msam_relpos_attention_backward": [_VP] * 8 + [_I] * 4 + [_F] + [_VP] * 7}


class HostBackend:
    """The C ABI of a host build on numpy arrays; every array sits between two guard zones that must come back bit-unchanged."""

    def __init__(self, lib):
        self.lib = lib
        for name, args in ABI.items():
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = ctypes.c_int32

    def _arr(self, shape, src=None):
        n = int(np.prod(shape))
        buf = np.full(n + 2 * GUARD, PATTERN if src is None else PATTERN_IN, np.uint32)
        view = buf[GUARD:GUARD + n].view(np.float32).reshape(shape)
        if src is not None:
            view[...] = src
        return buf, view

    def _call(self, fn, ins, dims, scale, out_shapes):
        bufs = [self._arr(a.shape, a) for a in ins] + [self._arr(s) for s in out_shapes]
        status = getattr(self.lib, fn)(*[v.ctypes.data for _, v in bufs[:len(ins)]], *dims, float(scale), *[v.ctypes.data for _, v in bufs[len(ins):]], None)
        assert status == 0, (fn, status)
        for i, (buf, _) in enumerate(bufs):
            pat = PATTERN_IN if i < len(ins) else PATTERN
            assert (buf[:GUARD] == pat).all() and (buf[-GUARD:] == pat).all(), f"{fn}: a guard zone was written"
        for (_, v), a in zip(bufs, ins):
            assert np.array_equal(v.view(np.uint32), a.view(np.uint32)), f"{fn}: an input was written"
        return [v.copy() for _, v in bufs[len(ins):]]

    def forward(self, c):
        if c.op == "plain":
            return self._call("msam_attention_forward", [c.q, c.k, c.v], (c.BH, c.Nq, c.Nk, c.D), c.scale, [(c.BH, c.Nq, c.D), (c.BH, c.Nq)])
        return self._call("msam_relpos_attention_forward", [c.q, c.k, c.v, c.bias_h, c.bias_w], (c.BH, c.Gh, c.Gw, c.D), c.scale,
                          [(c.BH, c.Nq, c.D), (c.BH, c.Nq)])

    def backward(self, c, out, lse):
        qs, ks = (c.BH, c.Nq, c.D), (c.BH, c.Nk, c.D)
        if c.op == "plain":
            names = ("dq", "dk", "dv", "delta")
            res = self._call("msam_attention_backward", [c.q, c.k, c.v, out, c.dout, lse], (c.BH, c.Nq, c.Nk, c.D), c.scale,
                             [qs, ks, ks, (c.BH, c.Nq)])
        else:
            names = ("dq", "dk", "dv", "dbias_h", "dbias_w", "delta")
            res = self._call("msam_relpos_attention_backward", [c.q, c.k, c.v, c.bias_h, c.bias_w, out, c.dout, lse],
                             (c.BH, c.Gh, c.Gw, c.D), c.scale, [qs, ks, ks, (c.BH, c.Nq, c.Gh), (c.BH, c.Nq, c.Gw), (c.BH, c.Nq)])
        return dict(zip(names, res))


def _source():
    return open(os.path.join(ROOT, "micro_sam_amd", "csrc", "train.hip")).read()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostBackend(shim.build_file(str(tmp_path_factory.mktemp("train_host")), ROOT, "train.hip", extra=shim.ERROR_STUBS))


def _host_cases(op):
    return [c for c in R.case_list(op) if c[3] not in ("peaked:first", "peaked:random")]


def _id(c):
    return f"{c[1][0]}x{c[1][1]}-D{c[2]}-{c[3]}{c[4] or ''}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest err / bound on the host:\n" + R.format_ratios("host"))


@pytest.mark.parametrize("case", _host_cases("plain"), ids=_id)
def test_plain_attention_table_on_the_cpu(host, case):
    c = R.make_case(*case)
    fails = R.check_case(c, R.run_case(host, c), "host")
    assert not fails, "\n".join(f[2] for f in fails)


@pytest.mark.parametrize("case", _host_cases("relpos"), ids=_id)
def test_relpos_attention_table_on_the_cpu(host, case):
    c = R.make_case(*case)
    fails = R.check_case(c, R.run_case(host, c), "host")
    assert not fails, "\n".join(f[2] for f in fails)


def test_the_table_covers_what_the_issue_names():
    """Every shape has both exact families and both kinds of bounded family; pi reaches every special key on the row-block shapes and
    at the LDS limit with a partial block."""
    for op, shapes in (("plain", R.PLAIN_SHAPES), ("relpos", R.RELPOS_SHAPES)):
        fams = {}
        for _, shape, D, fam, _ in R.case_list(op):
            fams.setdefault((shape, D), set()).add(fam)
        assert len(fams) == len(shapes) * 2
        assert all(f == {"uniform", "onehot", "diffuse", "peaked:last", "peaked:first", "peaked:random"} for f in fams.values())
    for op, shape, D in [("plain", s, 32) for s in R.ROWBLOCK_SHAPES] + [("relpos", (3, 64), 64)]:
        Nq, Nk = shape if op == "plain" else (192, 192)
        hit = set()
        for r in range(R.onehot_variants(op, Nq, Nk)):
            hit |= set(R.make_case(op, shape, D, "onehot", r).pi.reshape(-1).tolist())
        want = {0, Nk - 1} | ({255, 256, ((Nk - 1) // 256) * 256} if op == "plain" and Nk > 256 else set())
        assert want <= hit, (op, shape, sorted(want - hit))
    assert all(R.q_rows_route(*s) for s in [(1, 1024), (3, 1025), (64, 1279)]) and not any(R.q_rows_route(*s) for s in [(65, 1024), (64, 1023)])
    assert all(R.k_rows_route(*s) for s in [(1024, 1), (1025, 3), (1279, 64)]) and not any(R.k_rows_route(*s) for s in [(1024, 65), (1023, 64)])


def test_refusals_leave_the_outputs_alone(host):
    """Gw = 65 (over the LDS column array), D = 24 for plain attention, D = 32 for rel-pos: status 1, nothing written."""
    f = lambda *s: np.zeros(s, np.float32)
    lib = host.lib
    for fn, ins, dims, outs in (
            ("msam_relpos_attention_forward", [f(1, 65, 64)] * 3 + [f(1, 65, 1), f(1, 65, 65)], (1, 1, 65, 64), [(1, 65, 64), (1, 65)]),
            ("msam_relpos_attention_backward", [f(1, 65, 64)] * 3 + [f(1, 65, 1), f(1, 65, 65), f(1, 65, 64), f(1, 65, 64), f(1, 65)], (1, 1, 65, 64),
             [(1, 65, 64)] * 3 + [(1, 65, 1), (1, 65, 65), (1, 65)]),
            ("msam_attention_forward", [f(1, 4, 24)] * 3, (1, 4, 4, 24), [(1, 4, 24), (1, 4)]),
            ("msam_attention_backward", [f(1, 4, 24)] * 5 + [f(1, 4)], (1, 4, 4, 24), [(1, 4, 24)] * 3 + [(1, 4)]),
            ("msam_relpos_attention_forward", [f(1, 4, 32)] * 3 + [f(1, 4, 2), f(1, 4, 2)], (1, 2, 2, 32), [(1, 4, 32), (1, 4)]),
            ("msam_relpos_attention_backward", [f(1, 4, 32)] * 3 + [f(1, 4, 2), f(1, 4, 2), f(1, 4, 32), f(1, 4, 32), f(1, 4)], (1, 2, 2, 32),
             [(1, 4, 32)] * 3 + [(1, 4, 2), (1, 4, 2), (1, 4)])):
        bufs = [host._arr(s) for s in outs]
        status = getattr(lib, fn)(*[a.ctypes.data for a in ins], *dims, 0.125, *[v.ctypes.data for _, v in bufs], None)
        assert status == 1, fn
        assert all((b == PATTERN).all() for b, _ in bufs), fn


# ---- the mutation check

def _sub(old, new, count):
    def apply(src):
        assert src.count(old) == count, (old, src.count(old), count)
        return src.replace(old, new)
    return apply


_plain = lambda pred: (lambda c: c[0] == "plain" and pred(*c[1]))
_relpos = lambda c: c[0] == "relpos"
_FWD_DQ, _DK_DV = {"out", "lse", "delta", "dq", "dbias_h", "dbias_w"}, {"dk", "dv"}
# kernel form -> (the cases that run it, the outputs it writes)
SCOPES = {"thread forward / dQ": (_plain(lambda nq, nk: not R.q_rows_route(nq, nk)), _FWD_DQ),
          "row-block forward / dQ": (_plain(R.q_rows_route), _FWD_DQ),
          "thread dK / dV": (_plain(lambda nq, nk: not R.k_rows_route(nq, nk)), _DK_DV),
          "row-block dK / dV": (_plain(R.k_rows_route), _DK_DV),
          "rel-pos forward / dQ": (_relpos, _FWD_DQ), "rel-pos dK / dV": (_relpos, _DK_DV)}
# name -> (source edits, the kernel forms the edits touch: each must be reported by an exact assertion)
MUTATIONS = {
    "row-block loops drop their first stride": (
        [_sub("for (int j = threadIdx.x; j < Nk; j += 256)", "for (int j = threadIdx.x + 256; j < Nk; j += 256)", 2),
         _sub("for (int i = threadIdx.x; i < Nq; i += 256)", "for (int i = threadIdx.x + 256; i < Nq; i += 256)", 1)],
        ["row-block forward / dQ", "row-block dK / dV"]),
    "key loop bound Nk - 1": (
        [_sub("for (int j = 0; j < Nk; ++j)", "for (int j = 0; j < Nk - 1; ++j)", 2),
         _sub("for (int j = threadIdx.x; j < Nk; j += 256)", "for (int j = threadIdx.x; j < Nk - 1; j += 256)", 2)],
        ["thread forward / dQ", "row-block forward / dQ"]),
    "no rescale of the accumulator": ([_sub("acc[d] * a);", "acc[d]);", 3)], ["thread forward / dQ", "row-block forward / dQ", "rel-pos forward / dQ"]),
    "lse is the maximum alone": ([_sub("= m + __logf(l);", "= m;", 2), _sub("= M + __logf(L);", "= M;", 1)],
                                 ["thread forward / dQ", "row-block forward / dQ", "rel-pos forward / dQ"]),
    "r = 1 in the row-block merge": ([_sub("const float r = __expf(m - M);", "const float r = 1.f;", 1)], ["row-block forward / dQ"]),
    "dk without scale": ([_sub("dk[ro + d] = ak[d] * scale;", "dk[ro + d] = ak[d];", 2), _sub("dk[ro + d] = tk * scale;", "dk[ro + d] = tk;", 1)],
                         ["thread dK / dV", "row-block dK / dV", "rel-pos dK / dV"]),
    "kh and kw swapped in relpos_bwd_kv": ([_sub("const int kh = j / Gw, kw = j - kh * Gw;", "const int kh = j % Gw, kw = j / Gw;", 1)], ["rel-pos dK / dV"]),
    "dbias_w from the next column": ([_sub("dbias_w[row * Gw + kw] = sdbw[kw * 128 + threadIdx.x];",
                                           "dbias_w[row * Gw + kw] = sdbw[((kw + 1) % Gw) * 128 + threadIdx.x];", 1)], ["rel-pos forward / dQ"]),
    "no delta in dS": ([_sub("(dp - dl)", "(dp)", 3), _sub("(dp - delta[(long)bh * Nq + i])", "(dp)", 2), _sub("(dp - delta[row])", "(dp)", 1)],
                       ["thread forward / dQ", "row-block forward / dQ", "thread dK / dV", "row-block dK / dV", "rel-pos forward / dQ", "rel-pos dK / dV"]),
}


@pytest.fixture(scope="module")
def mutants(tmp_path_factory):
    base = _source()

    def build(item):
        name, (edits, _) = item
        src = base
        for e in edits:
            src = e(src)
        assert src != base
        return name, HostBackend(shim.build_file(str(tmp_path_factory.mktemp("mutant")), ROOT, "train.hip", source=src, extra=shim.ERROR_STUBS))

    with ThreadPoolExecutor(4) as ex:
        return dict(ex.map(build, MUTATIONS.items()))


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_is_reported_by_an_exact_assertion(mutants, name):
    exact = sorted((c for op in ("plain", "relpos") for c in R.case_list(op, bounded=False)), key=lambda c: c[1][0] * c[1][1] * c[2])
    for scope in MUTATIONS[name][1]:
        caught = None
        runs, outputs = SCOPES[scope]
        for case in filter(runs, exact):
            c = R.make_case(*case)
            hits = [f for f in R.check_case(c, R.run_case(mutants[name], c), "mutant") if f[0] == "exact" and f[1].replace("shift_", "") in outputs and "not finite" not in f[2]]
            if hits:
                caught = hits[0][2]
                break
        assert caught, f"'{name}' survives every exact case of the table in the {scope} kernels: the table is missing a case"
        print(f"{name} [{scope}]: {caught}")
