"""The calls HipBackend's K_nM pass wrappers (ktk, ktk2, ktkn, kvn, ktwn, trmvn, knm_mv) make into libodx, pinned without a
device: a wrong argument in one of these ctypes calls is an out-of-bounds access on the GPU, so it has to be catchable
before anything runs on one.

A HipBackend is made without a device (object.__new__ plus the attributes the wrappers read); its `lib` is a recording fake
whose *_workspace_bytes entries answer from a table and whose other entries log their call and return 0.  What is logged is
machine-independent: the entry, every scalar argument, and for every pointer argument the tensor it points into and the byte
offset (or null).  tests/golden/knm_calls.json holds the log of every case;
`PYTHONPATH=online-detection_amd python tests/test_knm_calls_host.py` writes it anew from the tree it runs in.

One stated normalisation: a plain entry (odx_knm_fwd_bwd, _q, odx_knm_fwd_bwd2, _q) is logged as its _t form with a null
t_out — in C both are one _impl and the plain entry passes t_out = nullptr.

The second half asks the real library — which answers *_workspace_bytes and odx_knm_pass_kernel_name without a GPU — over a
grid of shapes: a changed configuration rule, range count or support bound shows there.
"""
import ctypes
import json
import os
import types

import pytest
import torch

from odx import hip
from odx.backend import HipBackend, Knm, KnmStream, Precond

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knm_calls.json")
F64, F32 = torch.float64, torch.float32

# plain entry -> (its _t form, the position of t_out there)
_T_FORM = {"odx_knm_fwd_bwd": ("odx_knm_fwd_bwd_t", 7), "odx_knm_fwd_bwd2": ("odx_knm_fwd_bwd2_t", 8),
           "odx_knm_fwd_bwd_q": ("odx_knm_fwd_bwd_q_t", 10), "odx_knm_fwd_bwd2_q": ("odx_knm_fwd_bwd2_q_t", 11)}


class _FakeLib:
    """*_workspace_bytes: 64 + 16 sum((i + 1) arg_i) — every argument and its position count — or -3 where the fake has no
    such pass: the NV pass for nv <= width when width is 4 or 8, the two-vector passes when width >= 2, nothing in
    `unsupported`.  Every other entry: logged, returns 0."""

    def __init__(self, rec, width, unsupported):
        self._rec, self._width, self._unsupported = rec, width, set(unsupported)

    def _bytes(self, name, args):
        assert len(args) == len(hip.SIGNATURES[name][1]), name
        if name in self._unsupported:
            return -3
        if name == "odx_knm_fwd_bwdn_q_workspace_bytes" and not (self._width >= 4 and 3 <= args[3] <= self._width):
            return -3
        if name in ("odx_knm_fwd_bwd2_workspace_bytes", "odx_knm_fwd_bwd2_q_workspace_bytes") and self._width < 2:
            return -3
        if name == "odx_knm_fwdn_q_workspace_bytes":
            return 0
        return 64 + 16 * sum((i + 1) * int(a) for i, a in enumerate(args))

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *args: self._bytes(name, args)
        return lambda *args: self._rec.log(name, args)


class Rec:
    """One case: the named tensors, the backend over the fake library, and what it logged."""

    def __init__(self, width=8, unsupported=(), wide_pass_min=None):
        self.calls, self.ws, self.named = [], [], {}
        be = object.__new__(HipBackend)
        be.device = "cpu"
        be._stream = lambda: None
        be._workspace = self._workspace
        be.lib = _FakeLib(self, width, unsupported)
        be.wide_pass_min = wide_pass_min
        self.be = be

    # ---- tensors
    def t(self, name, tensor):
        self.named[name] = tensor
        return tensor

    def vec(self, name, n, dtype=F64):
        return self.t(name, torch.zeros(n, dtype=dtype))

    def mat(self, name, rows, cols, ld=None, skip=0, dtype=F64):
        """(rows, cols) view with leading dimension ld that starts `skip` elements into its buffer (skip = 1: rows that are
        not 16-byte aligned)."""
        ld = cols if ld is None else ld
        base = self.t(name, torch.zeros(rows * ld + skip + 2, dtype=dtype))
        return base.as_strided((rows, cols), (ld, 1), skip)

    def block(self, fmt, n, M, rows=None):
        """A stored block of n rows; rows = (lo, hi): that row range of it as a view (Knm.rows)."""
        K = Knm()
        K.n, K.M, K.fmt = n, M, fmt
        K.ld = (M + 3) // 4 * 4 if fmt == "f32" else (M + 7) // 8 * 8
        K.K = self.t("K", torch.zeros((n, K.ld), dtype=F32 if fmt == "f32" else torch.int16))
        if fmt == "u24":
            K.lo = self.t("Klo", torch.zeros((n, K.ld), dtype=torch.uint8))
        return K if rows is None else K.rows(*rows)

    def shard(self, n, M, D=24, ring=None):
        """A streamed shard (KnmStream) of n rows over M centres; ring: bytes of the caller's buffer, or None."""
        def feats(tag, rows):
            return types.SimpleNamespace(P=self.t(tag + ".P", torch.zeros((rows, 64), dtype=torch.int32)), n=rows, D=D,
                                         meta=self.vec(tag + ".meta", 2, F32), sq=self.vec(tag + ".sq", rows, F32))
        return KnmStream(feats("F", n), feats("Z", M), 1.5, None if ring is None else self.vec("ring", ring, torch.uint8))

    def precond(self, M):
        P = Precond()
        P.M, P.ld = M, (M + 1) // 2 * 2
        for name in ("LTi", "LTit", "LAi", "LAit"):
            setattr(P, name, self.t(name, torch.zeros((M, P.ld), dtype=F64)))
        return P

    # ---- logging
    def _workspace(self, key, nbytes):
        self.ws.append([key, int(nbytes)])
        return self.t("ws:" + key, torch.zeros(max(int(nbytes), 16), dtype=torch.uint8))

    def _where(self, p):
        if not p:
            return None
        for name, t in self.named.items():
            base = t.untyped_storage().data_ptr()
            if base <= p < base + max(t.untyped_storage().nbytes(), 1):
                return [name, p - base]
        return ["?", 0]          # a tensor the wrapper made itself

    def log(self, name, args):
        types_ = hip.SIGNATURES[name][1]
        assert len(args) == len(types_), "%s takes %d arguments, got %d" % (name, len(types_), len(args))
        out = []
        for a, ty in zip(args, types_):
            if ty is ctypes.c_void_p:
                assert a is None or isinstance(a, (int, ctypes.c_void_p)), "%s: pointer argument %r" % (name, a)
                out.append(self._where(getattr(a, "value", a)))
            elif ty is ctypes.c_double:
                assert isinstance(a, float), "%s: %r where a double goes" % (name, a)
                out.append(a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), "%s: %r where an integer goes" % (name, a)
                out.append(a)
        if name in _T_FORM:
            name, at = _T_FORM[name]
            out.insert(at, None)
        self.calls.append([name] + out)
        return 0

    def result(self, ret):
        """The log of the case, with what the wrapper returned (where each returned tensor lies, its shape and strides)."""
        rets = ret if isinstance(ret, tuple) else (ret,)
        desc = [[self._where(r.data_ptr()), list(r.shape), list(r.stride()), str(r.dtype)] for r in rets]
        return {"calls": self.calls, "workspaces": self.ws, "returns": desc}


# ------------------------------------------------------------------------------------------------------------- cases
N, M = 10, 21            # rows and columns of the blocks: neither a multiple of the plane's leading dimension (24 / 32)
CASES = {}


def case(name, **kw):
    def add(fn):
        assert name not in CASES
        CASES[name] = (fn, kw)
        return fn
    return add


def _any_block(r, fmt, n=N, rows=None, ring=None):
    return r.shard(n, M, ring=ring) if fmt == "stream" else r.block(fmt, n, M, rows=rows)


for _fmt in ("f32", "u24", "bf16", "stream"):
    for _how in ("v", "w", "vw") + (("t_out",) if _fmt != "stream" else ()):
        @case("ktk-%s-%s" % (_fmt, _how))
        def _(r, fmt=_fmt, how=_how):
            K = _any_block(r, fmt)
            return r.be.ktk(K, v=r.vec("v", M) if how != "w" else None, w=r.vec("w", N) if how in ("w", "vw") else None,
                            out=r.vec("out", M), t_out=r.vec("t", N) if how == "t_out" else None)

    @case("ktk-%s-out-none" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk(_any_block(r, fmt), v=r.vec("v", M))

    for _t in (False, True) if _fmt != "stream" else (False,):
        @case("ktk2-%s%s" % (_fmt, "-t_out" if _t else ""))
        def _(r, fmt=_fmt, t=_t):
            return r.be.ktk2(_any_block(r, fmt), r.vec("v1", M), r.vec("v2", M), out1=r.vec("o1", M), out2=r.vec("o2", M),
                             t_out=r.vec("t", N) if t else None)

    @case("ktk2-%s-out-none" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk2(_any_block(r, fmt), r.vec("v1", M), r.vec("v2", M))

for _fmt in ("f32", "u24", "bf16"):
    @case("ktk-%s-n0" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk(r.block(fmt, N, M, rows=(3, 3)), v=r.vec("v", M), out=r.vec("out", M))

    @case("ktk-%s-row-range" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk(r.block(fmt, N, M, rows=(3, 8)), v=r.vec("v", M), out=r.vec("out", M), t_out=r.vec("t", 5))

    @case("ktk2-%s-n0" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk2(r.block(fmt, N, M, rows=(3, 3)), r.vec("v1", M), r.vec("v2", M), out1=r.vec("o1", M), out2=r.vec("o2", M))


@case("ktk-stream-ring")
def _(r):
    return r.be.ktk(r.shard(N, M, ring=64), v=r.vec("v", M), out=r.vec("out", M))


@case("ktk2-stream-ring")
def _(r):
    return r.be.ktk2(r.shard(N, M, ring=64), r.vec("v1", M), r.vec("v2", M), out1=r.vec("o1", M), out2=r.vec("o2", M))


for _L in (1, 2, 3, 5, 8, 11):
    for _width in (8, 4, 2, 1):
        for _wmin in (None, 3):
            @case("ktkn-u24-L%d-w%d-min%s" % (_L, _width, _wmin), width=_width, wide_pass_min=_wmin)
            def _(r, L=_L):
                return r.be.ktkn(r.block("u24", N, M), r.mat("V", L, M, 24), out=r.mat("O", L, M, 26))
    for _fmt, _width, _wmin in (("bf16", 8, None), ("bf16", 2, 3), ("bf16", 1, 3), ("f32", 2, 3), ("f32", 1, None)):
        @case("ktkn-%s-L%d-w%d-min%s" % (_fmt, _L, _width, _wmin), width=_width, wide_pass_min=_wmin)
        def _(r, L=_L, fmt=_fmt):
            return r.be.ktkn(r.block(fmt, N, M), r.mat("V", L, M, 24), out=r.mat("O", L, M, 26))

for _L in (1, 2, 3, 16, 17, 18):
    @case("ktkn-stream-L%d" % _L)
    def _(r, L=_L):
        return r.be.ktkn(r.shard(N, M), r.mat("V", L, M, 24), out=r.mat("O", L, M, 26))


@case("ktkn-stream-ring-large-enough")
def _(r):
    return r.be.ktkn(r.shard(N, M, ring=4096), r.mat("V", 3, M, 24), out=r.mat("O", 3, M, 26))


@case("ktkn-stream-ring-too-small")
def _(r):
    return r.be.ktkn(r.shard(N, M, ring=64), r.mat("V", 3, M, 24), out=r.mat("O", 3, M, 26))


@case("ktkn-u24-out-none", width=8)
def _(r):
    return r.be.ktkn(r.block("u24", N, M), r.mat("V", 3, M, 24))


@case("ktkn-u24-n0-wide", width=2, wide_pass_min=3)
def _(r):
    return r.be.ktkn(r.block("u24", N, M, rows=(2, 2)), r.mat("V", 5, M, 24), out=r.mat("O", 5, M, 26))


@case("ktkn-u24-n0-nv", width=8)
def _(r):
    return r.be.ktkn(r.block("u24", N, M, rows=(2, 2)), r.mat("V", 5, M, 24), out=r.mat("O", 5, M, 26))


# rows that are not 16-byte aligned are refused for exactly the groups that need them: not for a pair or a single on a stored
# block, not for a single on a streamed shard, in ktwn or in trmvn
@case("ktkn-u24-pair-unaligned", width=2)
def _(r):
    return r.be.ktkn(r.block("u24", N, M), r.mat("V", 3, M, 25, skip=1), out=r.mat("O", 3, M, 27, skip=1))


@case("ktkn-stream-single-unaligned")
def _(r):
    return r.be.ktkn(r.shard(N, M), r.mat("V", 1, M, 25, skip=1), out=r.mat("O", 1, M, 27, skip=1))


@case("ktwn-u24-single-unaligned")
def _(r):
    return r.be.ktwn(r.block("u24", N, M), r.mat("W", 1, N, 11, skip=1), out=r.mat("O", 1, M, 27, skip=1))


@case("trmvn-single-unaligned")
def _(r):
    return r.be.trmvn(r.precond(M), "LTi", r.mat("X", 1, M, 25, skip=1), out=r.mat("O", 1, M, 27, skip=1))


@case("trmvn-out-and-z-unaligned")          # only X is asked to be aligned
def _(r):
    return r.be.trmvn(r.precond(M), "LAit", r.mat("X", 2, M, 24), alpha=2.0, beta=0.5, Z=r.mat("Z", 2, M, 25, skip=1),
                      out=r.mat("O", 2, M, 27, skip=1))


for _T in (1, 2, 8, 9):
    for _fmt in ("u24", "bf16"):
        @case("kvn-%s-T%d" % (_fmt, _T))
        def _(r, T=_T, fmt=_fmt):
            return r.be.kvn(r.block(fmt, N, M), r.mat("V", T, M, 24), out=r.mat("O", T, N, 12))

    for _fmt in ("u24", "bf16", "f32", "stream"):
        @case("ktwn-%s-T%d" % (_fmt, _T))
        def _(r, T=_T, fmt=_fmt):
            return r.be.ktwn(_any_block(r, fmt), r.mat("W", T, N, 12), out=r.mat("O", T, M, 26))

    for _name, _z in (("LTi", False), ("LTit", True), ("LAi", True), ("LAit", False)):
        @case("trmvn-%s-T%d" % (_name, _T))
        def _(r, T=_T, name=_name, z=_z):
            return r.be.trmvn(r.precond(M), name, r.mat("X", T, M, 24), alpha=0.25, beta=3.0 if z else 0.0,
                              Z=r.mat("Z", T, M, 28) if z else None, out=r.mat("O", T, M, 26))


@case("kvn-u24-out-none")
def _(r):
    return r.be.kvn(r.block("u24", N, M), r.mat("V", 3, M, 24))


@case("kvn-u24-n0")
def _(r):
    return r.be.kvn(r.block("u24", N, M, rows=(4, 4)), r.mat("V", 3, M, 24), out=r.mat("O", 3, 0, 2))


@case("ktwn-u24-out-none")
def _(r):
    return r.be.ktwn(r.block("u24", N, M), r.mat("W", 3, N, 12))


@case("ktwn-u24-n0")
def _(r):
    return r.be.ktwn(r.block("u24", N, M, rows=(4, 4)), r.mat("W", 3, 0, 2), out=r.mat("O", 3, M, 26))


@case("trmvn-out-none")
def _(r):
    return r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M, 24))


@case("trmvn-out-is-z")
def _(r):
    Z = r.mat("Z", 3, M, 28)
    return r.be.trmvn(r.precond(M), "LAi", r.mat("X", 3, M, 24), beta=1.0, Z=Z, out=Z)


for _fmt in ("f32", "u24", "bf16"):
    @case("knm_mv-%s" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.knm_mv(r.block(fmt, N, M), r.vec("alpha", M))

    @case("knm_mv-%s-strided-out" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.knm_mv(r.block(fmt, N, M), r.vec("alpha", M), out=r.mat("S", N, 7, dtype=F32)[:, 3:4])

    @case("knm_mv-%s-summed" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.knm_mv(r.block(fmt, N, M), None, summed=r.vec("sum", N))


@case("knm_mv-u24-vector-out")
def _(r):
    return r.be.knm_mv(r.block("u24", N, M), r.vec("alpha", M), out=r.vec("S", N, F32))


@case("knm_mv-u24-summed-strided-out")
def _(r):
    return r.be.knm_mv(r.block("u24", N, M), None, out=r.mat("S", N, 7, dtype=F32)[:, 3:4], summed=r.vec("sum", N))


@case("knm_mv-f32-alpha-f32")          # alpha in another type: converted by the wrapper, so not a named tensor
def _(r):
    return r.be.knm_mv(r.block("f32", N, M), r.vec("alpha", M, F32))


def _run(name):
    fn, kw = CASES[name]
    r = Rec(**kw)
    return r.result(fn(r))


_golden = None


def _load():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
    return _golden


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_are_the_recorded_ones(name):
    assert name in _load()["calls"], "no recorded calls for this case"
    assert json.loads(json.dumps(_run(name))) == _load()["calls"][name]


def test_the_fixture_has_no_other_cases():
    assert sorted(_load()["calls"]) == sorted(CASES)


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(exc, fn, match=None, **kw):
    r = Rec(**kw)
    with pytest.raises(exc, match=match):
        fn(r)
    return r


def test_t_out_is_checked():
    for fn in (lambda r: r.be.ktk(r.shard(N, M), v=r.vec("v", M), t_out=r.vec("t", N)),
               lambda r: r.be.ktk2(r.shard(N, M), r.vec("v1", M), r.vec("v2", M), t_out=r.vec("t", N)),
               lambda r: r.be.ktk(r.block("u24", N, M), w=r.vec("w", N), t_out=r.vec("t", N)),
               lambda r: r.be.ktk(r.block("u24", N, M), v=r.vec("v", M), t_out=r.vec("t", N + 1)),
               lambda r: r.be.ktk(r.block("f32", N, M), v=r.vec("v", M), t_out=r.vec("t", N, F32)),
               lambda r: r.be.ktk2(r.block("f32", N, M), r.vec("v1", M), r.vec("v2", M), t_out=r.mat("t", N, 2)[:, 0])):
        assert _refused(ValueError, fn).calls == []


@pytest.mark.parametrize("fmt", ["f32", "u24", "bf16"])
def test_a_block_without_a_pass_is_an_odx_error(fmt):
    q = "" if fmt == "f32" else "_q"
    r = _refused(hip.OdxError, lambda r: r.be.ktk(r.block(fmt, N, M), v=r.vec("v", M)),
                 unsupported=["odx_knm_fwd_bwd%s_workspace_bytes" % q])
    assert r.calls == [] and r.ws == []
    r = _refused(hip.OdxError, lambda r: r.be.ktk2(r.block(fmt, N, M), r.vec("v1", M), r.vec("v2", M)), width=1)
    assert r.calls == [] and r.ws == []
    assert not Rec(width=1).be.can_ktk2(Rec().block(fmt, N, M)) and Rec(width=2).be.can_ktk2(Rec().block(fmt, N, M))


def test_a_shard_outside_the_streamed_range_is_an_odx_error():
    for fn in (lambda r: r.be.ktk(r.shard(N, M), v=r.vec("v", M)),
               lambda r: r.be.ktk2(r.shard(N, M), r.vec("v1", M), r.vec("v2", M)),
               lambda r: r.be.ktkn(r.shard(N, M), r.mat("V", 1, M, 24))):
        r = _refused(hip.OdxError, fn, unsupported=["odx_gauss_ktk_stream_h2_workspace_bytes"])
        assert r.calls == [] and r.ws == []
    r = _refused(hip.OdxError, lambda r: r.be.ktkn(r.shard(N, M), r.mat("V", 3, M, 24)),
                 unsupported=["odx_gauss_ktk_stream_h2n_workspace_bytes"])
    assert r.calls == [] and r.ws == []
    assert Rec().be.can_ktk2(Rec().shard(N, M))


def test_ktkn_refusals():
    K = lambda r: r.block("u24", N, M)      # noqa: E731
    for fn in (lambda r: r.be.ktkn(K(r), r.mat("V", 3, M - 1, 24), out=r.mat("O", 3, M, 26)),          # too few columns
               lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 2, M, 26)),              # rows differ
               lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24, dtype=F32), out=r.mat("O", 3, M, 26)),
               lambda r: r.be.ktkn(K(r), r.mat("V", 3, 2 * M, 48)[:, ::2], out=r.mat("O", 3, M, 26)),  # rows not contiguous
               lambda r: r.be.ktkn(K(r), r.vec("V", M), out=r.mat("O", 1, M, 26)),
               lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24, skip=1), out=r.mat("O", 3, M, 26)),      # an nv group, unaligned
               lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 3, M, 27)),              # odd leading dimension
               lambda r: r.be.ktkn(r.shard(N, M), r.mat("V", 2, M, 24, skip=1), out=r.mat("O", 2, M, 26))):
        assert _refused(ValueError, fn).calls == []
    # a wide group, unaligned; the pass behind the wide route missing
    assert _refused(ValueError, lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 3, M, 26, skip=1)),
                    width=2, wide_pass_min=3).calls == []
    r = _refused(hip.OdxError, lambda r: r.be.ktkn(K(r), r.mat("V", 3, M, 24)), width=2, wide_pass_min=3,
                 unsupported=["odx_knm_bwdn_q_workspace_bytes"])
    assert [c[0] for c in r.calls] == ["odx_knm_fwdn_q"]
    r = _refused(ValueError, lambda r: r.be.ktkn(r.shard(N, M), r.mat("V", 18, M, 25, skip=1), out=r.mat("O", 18, M, 26)))
    assert r.calls == []


def test_kvn_refusals():
    for fmt in ("f32", "stream"):
        _refused(ValueError, lambda r: r.be.kvn(_any_block(r, fmt), r.mat("V", 3, M, 24)), match="compact")
    K = lambda r: r.block("u24", N, M)      # noqa: E731
    for fn in (lambda r: r.be.kvn(K(r), r.mat("V", 3, M - 1, 24)),
               lambda r: r.be.kvn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 3, N - 1, 12)),
               lambda r: r.be.kvn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 2, N, 12)),
               lambda r: r.be.kvn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 3, N, 12, dtype=F32)),
               lambda r: r.be.kvn(K(r), r.mat("V", 1, M, 24, skip=1)),            # even a single row
               lambda r: r.be.kvn(K(r), r.mat("V", 3, M, 24), out=r.mat("O", 3, N, 11))):
        assert _refused(ValueError, fn).calls == []
    r = _refused(hip.OdxError, lambda r: r.be.kvn(K(r), r.mat("V", 9, M, 24)), unsupported=["odx_knm_fwdn_q_workspace_bytes"])
    assert r.calls == []


def test_ktwn_refusals():
    K = lambda r: r.block("bf16", N, M)      # noqa: E731
    for fn in (lambda r: r.be.ktwn(K(r), r.mat("W", 3, N - 1, 12)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 3, N, 12), out=r.mat("O", 3, M - 1, 26)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 3, N, 12), out=r.mat("O", 4, M, 26)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 3, N, 12, dtype=F32)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 2, N, 12, skip=1)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 2, N, 12), out=r.mat("O", 2, M, 26, skip=1)),
               lambda r: r.be.ktwn(K(r), r.mat("W", 2, N, 11))):
        assert _refused(ValueError, fn).calls == []
    r = _refused(hip.OdxError, lambda r: r.be.ktwn(K(r), r.mat("W", 2, N, 12)), unsupported=["odx_knm_bwdn_q_workspace_bytes"])
    assert r.calls == [] and r.ws == []
    # a ninth row goes through ktk: the eight in front of it have run when that is refused
    r = _refused(hip.OdxError, lambda r: r.be.ktwn(K(r), r.mat("W", 9, N, 12)), unsupported=["odx_knm_fwd_bwd_q_workspace_bytes"])
    assert [c[0] for c in r.calls] == ["odx_knm_bwdn_q"]


def test_trmvn_refusals():
    for fn in (lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M - 1, 24)),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M, 24), out=r.mat("O", 2, M, 26)),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M, 24), beta=1.0, Z=r.mat("Z", 3, M - 1, 26)),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M, 24, dtype=F32)),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 3, M, 24), beta=1.0),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 2, M, 24, skip=1)),
               lambda r: r.be.trmvn(r.precond(M), "LTi", r.mat("X", 2, M, 25))):
        assert _refused(ValueError, fn).calls == []


def test_knm_mv_refusals():
    K = lambda r: r.block("u24", N, M)      # noqa: E731
    for fn in (lambda r: r.be.knm_mv(r.shard(N, M), r.vec("alpha", M)),
               lambda r: r.be.knm_mv(K(r), None, summed=r.vec("sum", N + 1)),
               lambda r: r.be.knm_mv(K(r), r.vec("alpha", M + 1)),
               lambda r: r.be.knm_mv(K(r), r.vec("alpha", M), out=r.vec("S", N)),                  # f64 out
               lambda r: r.be.knm_mv(K(r), r.vec("alpha", M), out=r.vec("S", N + 1, F32)),
               lambda r: r.be.knm_mv(K(r), r.vec("alpha", M), out=r.mat("S", N, 2, dtype=F32)),
               lambda r: r.be.knm_mv(K(r), None, out=r.vec("S", N), summed=r.vec("sum", N))):
        assert _refused(ValueError, fn).calls == []


# ---------------------------------------------------------------------------------- the real library's host geometry
GRID_M = (1, 4, 1021, 1024, 2524, 2528, 4097, 5084, 5088, 8192, 10000, 10240, 20440, 20441)
GRID_N = (0, 1, 7, 100000)
GRID_FMT = (("f32", hip.KNM_F32), ("u24", hip.KNM_U24), ("bf16", hip.KNM_BF16))


def _geometry():
    """entry -> the answers over the grid, in the order of the loops below."""
    lib = hip.load()
    g = {"fwd_bwd": [], "fwd_bwd2": [], "fwd_bwd_q": [], "fwd_bwd2_q": [], "fwd_bwdn_q": [], "bwdn_q": [], "fwdn_q": [],
         "kernel_name": []}
    for m in GRID_M:
        for _, code in GRID_FMT:
            g["kernel_name"].append([lib.odx_knm_pass_kernel_name(m, code, nv).decode() for nv in range(0, 10)])
        for n in GRID_N:
            g["fwd_bwd"].append(int(lib.odx_knm_fwd_bwd_workspace_bytes(n, m)))
            g["fwd_bwd2"].append(int(lib.odx_knm_fwd_bwd2_workspace_bytes(n, m)))
            for _, code in GRID_FMT:
                g["fwd_bwd_q"].append(int(lib.odx_knm_fwd_bwd_q_workspace_bytes(n, m, code)))
                g["fwd_bwd2_q"].append(int(lib.odx_knm_fwd_bwd2_q_workspace_bytes(n, m, code)))
                for entry in ("fwd_bwdn_q", "bwdn_q", "fwdn_q"):
                    fn = getattr(lib, "odx_knm_%s_workspace_bytes" % entry)
                    g[entry].append([int(fn(n, m, code, nv)) for nv in range(0, 10)])
    return g


def test_host_geometry_of_the_real_library():
    """Workspace sizes (configuration, workgroups per CU, row ranges: for the 256 compute units of an MI355X, which is also
    what the library assumes where it sees no device) and kernel names over GRID_M x GRID_N x formats x nv = 0 .. 9."""
    got = _geometry()
    want = _load()["geometry"]
    assert sorted(got) == sorted(want)
    for entry in got:
        assert got[entry] == want[entry], entry


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({"calls": {name: _run(name) for name in sorted(CASES)}, "geometry": _geometry()}, f, separators=(",", ":"),
                  sort_keys=True)
        f.write("\n")
