"""Every workspace of libodx held to what its *_workspace_bytes twin reports (tests/workspace_guard.py), on the MI355X.

A case is a small function prepare(be) -> op, op(be) -> tuple of tensors.  op runs three times on the same inputs: plainly
(the backend's ordinary, recycled workspaces, after release_workspaces()), under guarded(be, 0xFF) (every workspace exactly
as large as asked for, between two guard bands, every cell a NaN / -1) and under guarded(be, 0x5A) (every cell finite, huge
garbage).  Asserted: no OdxError (an ODX_ERR_WORKSPACE means query and entry disagree), both guard bands intact after both
guarded runs, the three outputs equal BIT FOR BIT (raw storage, K planes and the NaN cells behind `out=` buffers included;
the project asserts bitwise repeatability of all these operations elsewhere, so there is no tolerance), and the recorder saw
the queries the case claims.  Correctness against f64 is held by the other GPU modules; bitwise equality with the plain
run ties these cases to them.

COVERS maps every *_workspace_bytes name of include/odx.h to the ids of the cases that exercise it;
tests/test_workspace_guard_host.py asserts that its keys are exactly the header's names.

Shapes are the smallest that reach each layout (see the family comments).  There is no numerical constant here: the only
constants of this work are GUARD and the two poison bytes of tests/workspace_guard.py, which says why each was chosen.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workspace_guard as wg  # noqa: E402

pytestmark = pytest.mark.gpu


def Q(stem):
    return "odx_%s_workspace_bytes" % stem


class Case:
    def __init__(self, cid, queries, prepare, settings):
        self.id, self.queries, self.prepare, self.settings = cid, tuple(queries), prepare, dict(settings)


CASES = {}


def add(cid, queries, prepare, **settings):
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, queries, prepare, settings)


@pytest.fixture(scope="module")
def be():
    import odx
    odx.set_backend(None)
    b = odx.get_backend()
    yield b
    b.release_workspaces()
    _DATA.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- plumbing
_BE_ATTRS = ("native16", "wide_pass_min", "sigma_grid_min_features", "shared_mmv_min")
_HOOKS = ("rls_force_nt_gram", "t_inverse_force_stop")


@contextlib.contextmanager
def settings(be, kw):
    """Options of the table (gauss, knm_storage, h2_tile, precond), attributes of the backend and test hooks of the library for
    the three runs of a case, put back afterwards."""
    import odx
    kw = dict(kw)
    attrs = {k: kw.pop(k) for k in _BE_ATTRS if k in kw}
    hooks = {k: kw.pop(k) for k in _HOOKS if k in kw}
    with odx.options.override(**kw):
        try:
            for k, v in attrs.items():
                setattr(be, k, v)
            for k, v in hooks.items():
                odx.options.library_hook(k, v)
            yield
        finally:
            for k in attrs:
                vars(be).pop(k, None)           # (class attributes: the instance's override goes)
            for k in hooks:
                odx.options.library_hook(k, 0)


def _p(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def raw(t):
    """The tensor's elements as bytes (a view's own elements; hand over the base buffer to have the cells around it compared)."""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.contiguous().view(-1).view(torch.uint8)


def nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def kplanes(K):
    return (K.K,) if K.lo is None else (K.K, K.lo)


def run_case(be, case, offset16=False):
    with settings(be, case.settings):
        op = case.prepare(be)
        be.release_workspaces()
        outs = [[raw(t).clone() for t in op(be)]]
        torch.cuda.synchronize()
        for poison in wg.POISONS:
            with wg.guarded(be, poison, offset16=offset16) as g:
                got = [raw(t).clone() for t in op(be)]
                assert g.records or not case.queries, "the case took no workspace through the hook"
                if offset16:
                    assert all((buf.data_ptr() + wg.GUARD + wg.OFFSET) % 32 == 16 for _, _, buf in g.records)
                g.check()
            missing = set(case.queries) - g.asked()
            assert not missing, "claimed in COVERS but never asked: %s (asked: %s)" % (sorted(missing), sorted(g.asked()))
            outs.append(got)
        be.release_workspaces()
    plain, nan_run, big_run = outs
    assert len(plain) == len(nan_run) == len(big_run)
    for i, (a, b, c) in enumerate(zip(plain, nan_run, big_run)):
        assert a.shape == b.shape == c.shape, i
        if not (torch.equal(a, b) and torch.equal(a, c)):
            def where(x, y):
                diff = torch.nonzero(x != y).view(-1)
                return "equal" if diff.numel() == 0 else "%d of %d bytes differ (first %d, last %d)" % (int(diff.numel()), int(x.numel()), int(diff[0]), int(diff[-1]))
            raise AssertionError("output %d depends on what the workspace held: plain against 0xFF: %s; plain against 0x5A: %s; 0xFF against 0x5A: %s"
                                 % (i, where(a, b), where(a, c), where(b, c)))


# ---------------------------------------------------------------------------------------------------------------- data
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        _DATA[key] = make()
    return _DATA[key]


def _blob(N, D):
    """(X (N, D) f32 on the device, y (N,) f64 on the device): rows of tests.synth.blob_problem, made once per shape."""
    def make():
        from tests.synth import blob_problem
        X, y, _ = blob_problem(N, D, seed=7 * N + D)
        return torch.from_numpy(X).cuda(), torch.from_numpy(y.astype(np.float64)).cuda()
    return _cached(("blob", N, D), make)


def _centre_ids(N, M):
    return torch.from_numpy(np.sort(np.random.default_rng(N + 3 * M).permutation(N)[:M]).astype(np.int64)).cuda()


def problem(be, n, M, D, rows16=None):
    """F: the first n rows of a blob of max(n, M, 64) rows; Zf: M distinct rows of that blob; y, X (n, D) and the centre ids."""
    N = max(n, M, 64)                  # (a blob of one row has no spread to normalise by)
    X, y = _blob(N, D)
    idx = _centre_ids(N, M)
    Xo = X if rows16 is None else X.to(rows16)
    Fall = be.features(Xo)
    F = Fall if n == N else be.features(Xo[:n])
    return F, be.rows(Fall, idx), y[:n], X[:n], idx


def vectors(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((rows, cols), generator=g, dtype=torch.float64).cuda()


def even(n):
    return (n + 1) // 2 * 2


SIGMA = 10.0


def kernel_arg(kind):
    import odx
    return SIGMA if kind == "gauss" else odx.MaternKernel(SIGMA, {"m32": 1.5, "m52": 2.5}[kind])


# ---------------------------------------------------------------------------------------------------------------- builds
# (n, M, D): 513 = 3 row blocks of 256 -> one phantom block in the launch's band of 4, an odd M, D no multiple of 64;
# 1025 = 5 row blocks -> 3 phantom blocks; and the smallest block there is.
BUILD_SHAPES = [(513, 257, 70), (1025, 130, 36), (1, 1, 8)]
BUILD_CONFIGS = [   # name, kernel, 16-bit rows, claimed query, settings
    ("f32-t256", "gauss", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="f32", h2_tile=256)),
    ("f32-t128", "gauss", None, Q("knm_fwd_bwd"), dict(knm_storage="f32", h2_tile=128)),          # (the build, then one pass for K' w)
    ("u24-t256", "gauss", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="u24", h2_tile=256)),
    ("bf16-t256", "gauss", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="bf16", h2_tile=256)),
    ("m32-f32", "m32", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="f32")),
    ("m32-u24", "m32", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="u24")),
    ("m52-f32", "m52", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="f32")),
    ("m52-bf16", "m52", None, Q("gauss_knm_h2_rhs"), dict(knm_storage="bf16")),
    ("rows-bf16-f32", "gauss", torch.bfloat16, Q("gauss_knm_b16_store"), dict(knm_storage="f32", h2_tile=256, native16=True)),
    ("rows-bf16-u24", "gauss", torch.bfloat16, Q("gauss_knm_b16_store"), dict(knm_storage="u24", h2_tile=256, native16=True)),
    ("rows-f16-f32", "gauss", torch.float16, Q("gauss_knm_b16_store"), dict(knm_storage="f32", h2_tile=256, native16=True)),
    ("rows-f16-bf16", "gauss", torch.float16, Q("gauss_knm_b16_store"), dict(knm_storage="bf16", h2_tile=256, native16=True)),
]


def _build(n, M, D, kind, rows16, be):
    F, Zf, y, _, _ = problem(be, n, M, D, rows16)
    w = y * (1.0 / n)
    sigma = kernel_arg(kind)

    def op(be):
        rhs = nan64(M + 4)
        K, _ = be.knm_rhs(F, Zf, sigma, w, rhs_out=rhs[:M])
        return kplanes(K) + (rhs,)
    return op


for _n, _M, _D in BUILD_SHAPES:
    for _name, _kind, _r16, _q, _set in BUILD_CONFIGS:
        add("build-%s-%dx%dx%d" % (_name, _n, _M, _D), [_q], functools.partial(_build, _n, _M, _D, _kind, _r16), **_set)


def _build_sigmas(n, M, D, be):
    F, Zf, y, _, _ = problem(be, n, M, D)
    w = y * (1.0 / n)

    def op(be):
        res = be.knm_rhs_sigmas(F, Zf, [4.0, 8.0, 12.0], w)
        return tuple(t for K, b in res for t in kplanes(K) + (b,))
    return op


for _fmt in ("f32", "u24"):
    add("build-sigmas-%s-513x257x70" % _fmt, [Q("gauss_knm_h2_store_sigmas")], functools.partial(_build_sigmas, 513, 257, 70),
        knm_storage=_fmt, h2_tile=256, sigma_grid_min_features=0)


# ---------------------------------------------------------------------------------------------------------------- scoring
# n = 1 and 513: an odd n (round_up(n, 2) is the slab's leading dimension), 3 row blocks against the launch's 8;
# M = 70 and 1300: 1300 is 6 wide (256) and 11 narrow (128) column tiles, so the two cores group differently;
# T = 1, 3, 9: 9 crosses a group of 8 columns.
SCORE_D = 70


def _block_columns(M, T):
    """(V (M, T) with column c non-zero on its own range only, ranges (T, 2) int32): ranges of different lengths and starts."""
    V = vectors(M, T, 11 * M + T)
    ranges = []
    for c in range(T):
        lo, hi = (c * M) // (2 * T), M - ((T - 1 - c) * M) // (3 * T)
        V[:lo, c] = 0.0
        V[hi:, c] = 0.0
        ranges.append([lo, hi])
    return V, torch.tensor(ranges, dtype=torch.int32, device="cuda")


def _score(n, M, T, route, kind, rows16, be):
    F, Zf, _, _, _ = problem(be, n, M, SCORE_D, rows16)
    sigma = kernel_arg(kind)
    if route == "ranges":
        V, ranges = _block_columns(M, T)
        return lambda be: (be.mmv(F, Zf, sigma, V, ranges=ranges),)
    V = vectors(M, T, 13 * M + T)
    if route == "sigmas":
        widths = [6.0 + 1.5 * c for c in range(T)]
        return lambda be: (be.mmv_sigmas(F, Zf, widths, V),)
    return lambda be: (be.mmv(F, Zf, sigma, V),)           # "dense": the shared-centre route from two columns on, else mmv's own


def _score_id(route, kind, tile, n, M, T):
    return "score-%s-%s-t%d-%dx%dx%d" % (route, kind, tile, n, M, T)


for _tile in (128, 256, 0):
    for _n in (1, 513):
        for _M in (70, 1300):
            for _T in (1, 3, 9):
                add(_score_id("ranges", "gauss", _tile, _n, _M, _T), [Q("gauss_mmv_h2")],
                    functools.partial(_score, _n, _M, _T, "ranges", "gauss", None), gauss="h2", h2_tile=_tile)
                if _T > 1:
                    add(_score_id("dense", "gauss", _tile, _n, _M, _T), [Q("gauss_mmvn_h2")],
                        functools.partial(_score, _n, _M, _T, "dense", "gauss", None), gauss="h2", h2_tile=_tile)
    # one layout each of the other routes per tile pin: the odd n against the wide M and a group of 8 crossed, and the smallest call
    for _n, _M, _T in ((513, 1300, 9), (1, 70, 3)):
        add(_score_id("sigmas", "gauss", _tile, _n, _M, _T), [Q("gauss_mmvn_h2_sigmas")],
            functools.partial(_score, _n, _M, _T, "sigmas", "gauss", None), gauss="h2", h2_tile=_tile)
        for _dt, _dn in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
            add(_score_id("ranges", "rows" + _dn, _tile, _n, _M, _T), [Q("gauss_mmv_b16")],
                functools.partial(_score, _n, _M, _T, "ranges", "gauss", _dt), gauss="h2", h2_tile=_tile, native16=True)
            add(_score_id("dense", "rows" + _dn, _tile, _n, _M, _T), [Q("gauss_mmvn_b16")],
                functools.partial(_score, _n, _M, _T, "dense", "gauss", _dt), gauss="h2", h2_tile=_tile, native16=True)

# the Matern kinds run on the wide core at every shape, in a slab sized by the 128-tile grouping's query: every shape, no pin
for _kind in ("m32", "m52"):
    for _n in (1, 513):
        for _M in (70, 1300):
            for _T in (1, 3, 9):
                add(_score_id("ranges", _kind, 0, _n, _M, _T), [Q("gauss_mmv_h2")],
                    functools.partial(_score, _n, _M, _T, "ranges", _kind, None), gauss="h2")
                if _T > 1:
                    add(_score_id("dense", _kind, 0, _n, _M, _T), [Q("gauss_mmvn_h2")],
                        functools.partial(_score, _n, _M, _T, "dense", _kind, None), gauss="h2")

# the e4m3 route (odx_gauss_mmv_f8) is sized by the split kernels' query
for _n, _M, _T in ((513, 1300, 9), (513, 70, 3), (1, 1300, 1), (1, 70, 3)):
    add(_score_id("dense", "f8", 0, _n, _M, _T), [Q("gauss_mmv_h2")], functools.partial(_score, _n, _M, _T, "dense", "gauss", None), gauss="f8")
    add(_score_id("ranges", "f8", 0, _n, _M, _T), [Q("gauss_mmv_h2")], functools.partial(_score, _n, _M, _T, "ranges", "gauss", None), gauss="f8")


def _score_short_ranges(kind, be):
    """Per-column ranges whose max_range (400) is well below Mtot (1300): the slab is sized by max_range."""
    n, M, T = 513, 1300, 3
    F, Zf, _, _, _ = problem(be, n, M, SCORE_D)
    V = vectors(M, T, 5)
    ranges = torch.tensor([[0, 200], [300, 700], [910, 1300]], dtype=torch.int32, device="cuda")
    for c, (lo, hi) in enumerate(ranges.tolist()):
        V[:lo, c] = 0.0
        V[hi:, c] = 0.0
    sigma = kernel_arg(kind)
    return lambda be: (be.mmv(F, Zf, sigma, V, ranges=ranges, max_range=400),)


def _score_strided_out(route, be):
    """out= a column block of a wider NaN-filled matrix: the cells beside it stay NaN."""
    n, M, T = 513, 1300, 3
    F, Zf, _, _, _ = problem(be, n, M, SCORE_D)
    V, ranges = _block_columns(M, T)

    def op(be):
        buf = nan32(n + 1, T + 5)
        be.mmv(F, Zf, SIGMA, V, ranges=ranges if route == "ranges" else None, out=buf[:n, 2:2 + T])
        return (buf,)
    return op


for _tile in (128, 256):
    add("score-short-ranges-gauss-t%d" % _tile, [Q("gauss_mmv_h2")], functools.partial(_score_short_ranges, "gauss"), gauss="h2", h2_tile=_tile)
    add("score-strided-out-ranges-t%d" % _tile, [Q("gauss_mmv_h2")], functools.partial(_score_strided_out, "ranges"), gauss="h2", h2_tile=_tile)
    add("score-strided-out-dense-t%d" % _tile, [Q("gauss_mmvn_h2")], functools.partial(_score_strided_out, "dense"), gauss="h2", h2_tile=_tile)
add("score-short-ranges-m52", [Q("gauss_mmv_h2")], functools.partial(_score_short_ranges, "m52"), gauss="h2")


# ---------------------------------------------------------------------------------------------------------------- passes over stored blocks
# M: both LDS limits of the NV passes and both sides of each (2524 | 2525: 8 vectors, 5084 | 5085: 4 vectors), the
# two-vector pass's last width (10000), a small odd width and the widest supported (20440).  n = 333: odd, two row blocks
# of most configurations, within the 200 .. 530 of the existing pass tests.
PASS_N = 333
PASS_MS = (129, 2524, 2525, 5084, 5085, 10000, 20440)
PASS_NVS = (1, 3, 5, 8, 11)


def stored_block(be, fmt, n, M):
    """A random stored block in the library's layout (pad columns zero), made once per (fmt, n, M)."""
    def make():
        g = torch.Generator().manual_seed(n + 3 * M)
        K = be._knm_block(n, M, fmt, None)
        K.K.zero_()
        if fmt == "f32":
            K.K[:, :M] = torch.rand((n, M), generator=g).cuda()
        elif fmt == "u24":
            K.lo.zero_()
            K.K[:, :M] = torch.randint(-32768, 32768, (n, M), generator=g, dtype=torch.int16).cuda()
            K.lo[:, :M] = torch.randint(0, 256, (n, M), generator=g, dtype=torch.uint8).cuda()
        else:
            K.K[:, :M] = torch.rand((n, M), generator=g).to(torch.bfloat16).view(torch.int16).cuda()
        return K
    return _cached(("block", fmt, n, M), make)


def _pass12(fmt, M, be):
    """The one- and two-vector passes: ktk with v, w and t_out, ktk with w alone, ktk2 with t_out where it exists."""
    n = PASS_N
    K = stored_block(be, fmt, n, M)
    V = vectors(2, even(M), M)[:, :M]                 # (each row starts on 16 bytes)
    w = vectors(1, n, M + 1)[0]

    def op(be):
        o1, t1, o2 = nan64(M + 4), nan64(n + 2), nan64(M + 4)
        be.ktk(K, v=V[0], w=w, out=o1[:M], t_out=t1[:n])
        be.ktk(K, w=w, out=o2[:M])
        res = (o1, t1, o2)
        if be.can_ktk2(K):
            a, b, t2 = nan64(M + 4), nan64(M + 4), nan64(n + 2)
            be.ktk2(K, V[0], V[1], out1=a[:M], out2=b[:M], t_out=t2[:n])
            res += (a, b, t2)
        return res
    return op


for _M in PASS_MS:
    _Mf = min(_M, 20000)             # (the f32 pass's widest configuration; the compact passes go on to 20440)
    add("pass12-f32-%d" % _Mf, [Q("knm_fwd_bwd"), Q("knm_fwd_bwd2")], functools.partial(_pass12, "f32", _Mf))
    for _fmt in ("u24", "bf16"):
        add("pass12-%s-%d" % (_fmt, _M), [Q("knm_fwd_bwd_q"), Q("knm_fwd_bwd2_q")], functools.partial(_pass12, _fmt, _M))


def _pass_mapped(fmt, Md, be):
    """A block of DISTINCT columns with its column map: vectors of the centre list's length (Md + 5) over Md stored columns; the
    two-vector pass where the width has one (4097 .. 10001 columns)."""
    from odx.backend import Knm
    from odx.cols import column_map
    n = PASS_N
    idx = np.concatenate([np.arange(Md), [0, 0, 0, 5, 77]]).astype(np.int64)
    np.random.default_rng(3).shuffle(idx)
    cmap = column_map(torch.from_numpy(idx))
    assert (cmap.Mv, cmap.Md) == (Md + 5, Md)
    Kd = stored_block(be, fmt, n, Md)
    Km = Knm()
    Km.K, Km.lo, Km.n, Km.M, Km.ld, Km.fmt = Kd.K, Kd.lo, Kd.n, Kd.M, Kd.ld, Kd.fmt
    Km.cmap, Km.Mv = cmap, cmap.Mv
    Mv = cmap.Mv
    V = vectors(2, even(Mv), 17)[:, :Mv]
    w = vectors(1, n, 18)[0]

    def op(be):
        o1, t1, a, b, t2 = nan64(Mv + 4), nan64(n + 2), nan64(Mv + 4), nan64(Mv + 4), nan64(n + 2)
        be.ktk(Km, v=V[0], w=w, out=o1[:Mv], t_out=t1[:n])
        if be.can_ktk2(Km):
            be.ktk2(Km, V[0], V[1], out1=a[:Mv], out2=b[:Mv], t_out=t2[:n])
        return (o1, t1, a, b, t2)
    return op


for _fmt in ("u24", "bf16"):
    for _Md in (129, 5085):
        add("pass12-mapped-%s-%d" % (_fmt, _Md), [Q("knm_fwd_bwd_q"), Q("knm_fwd_bwd2_q")], functools.partial(_pass_mapped, _fmt, _Md))


def _passn(fmt, M, nv, be):
    """ktkn, ktwn, kvn and ktkn_rows (with and without t_out) over nv vectors.  wide_pass_min = 3 sends ktkn's groups of three and
    more through the two-read route above M = 5084, whose T is a Python-level view of the "ktkn_t" workspace; ktkn_rows takes
    that route there whatever the attribute says, and its weighted copy W is the same workspace."""
    n = PASS_N
    K = stored_block(be, fmt, n, M)
    ldm, ldn = even(M), even(n)
    V = vectors(nv, ldm, M + nv)
    W = vectors(nv, ldn, M + nv + 1)
    Dw = vectors(2, ldn, M + nv + 2).abs()
    wrow = [(-1, 0, 1)[l % 3] for l in range(nv)]

    def op(be):
        o1 = be.ktkn(K, V, out=nan64(nv, ldm + 2)[:, :ldm])
        o2 = be.ktwn(K, W, out=nan64(nv, ldm + 2)[:, :ldm])
        o3 = be.kvn(K, V, out=nan64(nv, ldn + 2)[:, :ldn])
        t = nan64(nv, ldn + 2)[:, :ldn]
        o4 = be.ktkn_rows(K, V, Dw, wrow, out=nan64(nv, ldm + 2)[:, :ldm], t_out=t)
        o5 = be.ktkn_rows(K, V, Dw, wrow)
        return tuple(x._base if x._base is not None else x for x in (o1, o2, o3, t, o4)) + (o5[:, :M],)
    return op


for _fmt in ("u24", "bf16"):
    for _M in PASS_MS:
        for _nv in PASS_NVS:
            add("passn-%s-%d-nv%d" % (_fmt, _M, _nv),
                [Q("knm_fwdn_q"), Q("knm_fwd_bwdn_q"), Q("knm_fwd_bwdn_q_rw"), Q("knm_bwdn_q") if _nv >= 2 else Q("knm_fwd_bwd_q")],
                functools.partial(_passn, _fmt, _M, _nv), wide_pass_min=3)


# ---------------------------------------------------------------------------------------------------------------- streamed shards
def _stream_shape(be, M, D, tail):
    if tail is None:
        return 777
    return 2 * int(be.lib.odx_gauss_ktk_stream_h2n_rows(M, D)) + tail         # two whole chunks and a ragged one, as PASS_SHAPES


def _stream(M, D, sigma, tail, small_ring, be):
    """ktk / ktk2 / ktkn on a shard that is never stored: the ring is the workspace.  small_ring: the caller's ring cannot hold the
    several-vector entry's layout, so the backend's workspace serves (and the caller's ring is never written)."""
    from odx.backend import KnmStream
    n = _stream_shape(be, M, D, tail)
    F, Zf, _, _, _ = problem(be, n, M, D)
    be.pack(F), be.pack(Zf)
    ldm = even(M)
    V = vectors(16, ldm, M + D)
    w = vectors(1, n, M + D + 1)[0]

    def op(be):
        if small_ring:
            ring = torch.zeros(4096, dtype=torch.uint8, device="cuda")
            S = KnmStream(F, Zf, sigma, ring)
            return (be.ktkn(S, V[:5], out=nan64(5, ldm)), ring)
        S = KnmStream(F, Zf, sigma, None)
        o1, a, b = nan64(M + 4), nan64(M + 4), nan64(M + 4)
        be.ktk(S, v=V[0, :M], w=w, out=o1[:M])
        be.ktk2(S, V[0, :M], V[1, :M], out1=a[:M], out2=b[:M])
        return (o1, a, b, be.ktkn(S, V[:5], out=nan64(5, ldm)), be.ktkn(S, V, out=nan64(16, ldm)), be.ktkn(S, V[:1], out=nan64(1, ldm)))
    return op


for _M, _D, _sig, _tail in ((129, 36, 5.0, None), (300, 64, 4.0, 777)):        # (777, 129, 36), and PASS_SHAPES[0] of test_gpu_stream_path
    _tag = "%dx%d%s" % (_M, _D, "" if _tail is None else "-ragged")
    add("stream-own-ring-%s" % _tag, [Q("gauss_ktk_stream_h2"), Q("gauss_ktk_stream_h2n")], functools.partial(_stream, _M, _D, _sig, _tail, False),
        gauss="h2")
    add("stream-small-ring-%s" % _tag, [Q("gauss_ktk_stream_h2n")], functools.partial(_stream, _M, _D, _sig, _tail, True), gauss="h2")


# ---------------------------------------------------------------------------------------------------------------- preconditioners
LAM, EPS = 1e-4, 1e-5


def _centres_only(be, M, D):
    X, _ = _blob(max(M, 64), D)
    return be.features(X[:M])


def _precond(M, D, kind, be):
    Zf = _centres_only(be, M, D)
    sigma = kernel_arg(kind)

    def op(be):
        out = nan64(4, M, even(M))
        P = be.precond(Zf, sigma, LAM, EPS, out=out)
        return (out, P.info)
    return op


for _M in (7, 130, 257):
    for _kind in ("gauss", "m32", "m52"):
        add("precond-%s-%d" % (_kind, _M), [Q("falkon_precond")], functools.partial(_precond, _M, 36, _kind))
add("precond-gauss-4100-split", [Q("falkon_precond")], functools.partial(_precond, 4100, 64, "gauss"))      # the shipped rule: split-f16 chain


def _precond_batched(Ms, D, t_stop, be):
    X, _ = _blob(2 * max(Ms), D)
    Zs = [be.features(X[17 * b:17 * b + M]) for b, M in enumerate(Ms)]
    Mmax = max(Ms)

    def op(be):
        out = nan64(len(Ms), 4, Mmax, even(Mmax))
        Ps = be.precond_batched(Zs, SIGMA, LAM, EPS, out=out, t_stop=t_stop)
        return (out, torch.cat([P.info for P in Ps]))
    return op


add("precond-batched-ragged", [Q("falkon_precond_batched")], functools.partial(_precond_batched, [130, 257, 64], 36, 0))
add("precond-batched-partial-t-inverse", [Q("falkon_precond_batched")], functools.partial(_precond_batched, [600, 300], 36, 256))


def _precond_path(M, D, kind, be):
    Zf = _centres_only(be, M, D)
    sigma = kernel_arg(kind)
    lams = [1e-3, 1e-4, 1e-5]

    def op(be):
        out = nan64(2 + 2 * len(lams), M, even(M))
        Ps = be.precond_path(Zf, sigma, lams, EPS, out=out)
        return (out, torch.cat([P.info for P in Ps]))
    return op


add("precond-path-gauss-257", [Q("falkon_precond_path")], functools.partial(_precond_path, 257, 36, "gauss"))
add("precond-path-m32-130", [Q("falkon_precond_path")], functools.partial(_precond_path, 130, 36, "m32"))


def _tri_blocked(M, t_stop, be):
    """The products with a PARTIAL inverse of T (block boundaries every t_stop rows), both orientations."""
    Zf = _centres_only(be, M, 36)
    P = be.precond_batched([Zf], SIGMA, LAM, EPS, t_stop=t_stop)[0]
    assert P.blocks and len(P.blocks) >= 3
    x, z = vectors(1, M, M)[0], vectors(1, M, M + 1)[0]

    def op(be):
        a, b = nan64(M + 4), nan64(M + 4)
        be.trmv(P, "LTi", x, alpha=0.5, beta=2.0, z=z, out=a[:M])
        be.trmv(P, "LTit", x, out=b[:M])
        return (a, b)
    return op


add("tri-blocked-mv-129", [Q("tri_blocked_mv")], functools.partial(_tri_blocked, 129, 128))
add("tri-blocked-mv-1000", [Q("tri_blocked_mv")], functools.partial(_tri_blocked, 1000, 256))


def _potrf_trtri(M, be):
    """odx_potrf_f64 and odx_trtri_f64 directly (the backend reaches them only inside the chains): workspaces through the hook."""
    from odx import hip
    ld = even(M)
    G = vectors(M, M + 20, M)
    A = torch.zeros((M, ld), dtype=torch.float64, device="cuda")
    A[:, :M] = torch.tril(G @ G.t() / (M + 20) + 0.1 * torch.eye(M, dtype=torch.float64, device="cuda"))

    def op(be):
        dA = A.clone()
        info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        ws = be._workspace("potrf", be.lib.odx_potrf_workspace_bytes(M))
        hip.check(be.lib.odx_potrf_f64(_p(dA), ld, M, _p(info), _p(ws), ws.numel(), be._stream()), "odx_potrf_f64")
        Li, Lit = nan64(M, ld), nan64(M, ld)
        ws2 = be._workspace("trtri", be.lib.odx_trtri_workspace_bytes(M))
        hip.check(be.lib.odx_trtri_f64(_p(dA), ld, M, _p(Li), _p(Lit), ld, _p(ws2), ws2.numel(), be._stream()), "odx_trtri_f64")
        return (dA, info, Li, Lit)
    return op


for _M in (129, 300, 1537):
    add("potrf-trtri-%d" % _M, [Q("potrf"), Q("trtri")], functools.partial(_potrf_trtri, _M))


# ---------------------------------------------------------------------------------------------------------------- CG loops
def _solver_options():
    from odx.solver import SolverOptions
    return SolverOptions(check_pivots=False)


def _cg_solve(n, M, D, be):
    F, Zf, y, _, _ = problem(be, n, M, D)
    opt = _solver_options()
    K, b0 = be.knm_rhs(F, Zf, SIGMA, y * (1.0 / n))
    assert K.fmt == "f32"
    P = be.precond(Zf, SIGMA, LAM, opt.pc_epsilon)
    return lambda be: (be.cg_solve(K, P, b0.clone(), n, LAM, 10, opt),)


add("cg-solve-777x129", [Q("falkon_cg")], functools.partial(_cg_solve, 777, 129, 36), knm_storage="f32")


def _cg_batched(specs, D, be):
    """Two classes of different n and M in one lock-step loop (one pass configuration)."""
    opt = _solver_options()
    Fs, Zfs, ys = [], [], []
    for n, M in specs:
        F, Zf, y, _, _ = problem(be, n, M, D)
        Fs.append(F), Zfs.append(Zf), ys.append(y)
    Ps = be.precond_batched(Zfs, SIGMA, LAM, opt.pc_epsilon)
    Mmax = max(M for _, M in specs)
    b0s = torch.zeros((len(specs), even(Mmax)), dtype=torch.float64, device="cuda")
    Ks = [be.knm_rhs(F, Zf, SIGMA, y * (1.0 / F.n), rhs_out=b0s[i, :Zf.n])[0] for i, (F, Zf, y) in enumerate(zip(Fs, Zfs, ys))]

    def op(be):
        alphas = be.cg_solve_batched(Ks, Ps, b0s, [F.n for F in Fs], LAM, 10, opt)
        assert alphas is not None
        return (alphas,)
    return op


_CG_SPECS = [(777, 129), (401, 257)]
add("cg-batched-f32", [Q("falkon_cg_batched")], functools.partial(_cg_batched, _CG_SPECS, 36), knm_storage="f32")
for _fmt in ("u24", "bf16"):
    add("cg-batched-%s" % _fmt, [Q("falkon_cg_batched_q")], functools.partial(_cg_batched, _CG_SPECS, 36), knm_storage=_fmt, h2_tile=256)


# ---------------------------------------------------------------------------------------------------------------- RLS
def _rls_single(D, nc, be):
    from tests import rls_checks as rc
    b = rc.Batch(D, [nc], seed=D + nc)
    F = be.row_matrix(torch.from_numpy(b.X).cuda())
    idx, Yt = torch.from_numpy(b.rows[0]).cuda(), torch.from_numpy(b.Yt).cuda()
    D1, ld = D + 1, even(D + 1)

    def op(be):
        G = torch.zeros((D1, ld), dtype=torch.float64, device="cuda")
        XtY = torch.zeros((4, ld), dtype=torch.float64, device="cuda")
        be.rls_gram(F, idx, Yt, G, XtY)
        W, info = be.rls_solve(G, D, 10.0, XtY)
        return (G, XtY, W[:, :D1], info)
    return op


def _rls_batched(D, be):
    """Three classes of 5, 130 and 0 rows: the Grams with the targets in one call, then the same from Grams begun alone."""
    from tests import rls_checks as rc
    b = rc.Batch(D, [5, 130, 0], seed=D)
    F = be.row_matrix(torch.from_numpy(b.X).cuda())
    idx_pad = be.rls_pad_index(torch.from_numpy(b.run).cuda(), b.seg_off, b.lengths, b.npad)[0]
    Yt = torch.from_numpy(b.Yt).cuda()
    D1 = D + 1

    def op(be):
        W, info = be.rls_train_batched(F, idx_pad, b.seg_off, b.lengths, Yt, 10.0)
        res = (W[:, :, :D1], info)
        if be.rls_rows_form(F):
            G = be.rls_gram_begin(F, idx_pad, b.seg_off, b.lengths, be.rls_gram_zeros(F, b.C))
            W2, info2 = be.rls_train_batched(F, idx_pad, b.seg_off, b.lengths, Yt, 10.0, begun=G)
            res += (W2[:, :, :D1], info2)
        return res
    return op


for _D in (36, 64, 70):          # 64: the Grams from the rows; 36 and 70 (D % 8 != 0): the transposed copy + NT GEMM
    add("rls-single-D%d" % _D, [Q("rls_gram"), Q("rls_solve")], functools.partial(_rls_single, _D, 130))
    add("rls-batched-D%d" % _D, [Q("rls_gram_batched"), Q("rls_solve_batched")], functools.partial(_rls_batched, _D))


# ---------------------------------------------------------------------------------------------------------------- NMS
def _boxes(R, seed):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand((R, 2), generator=g) * 400
    wh = torch.rand((R, 2), generator=g) * 120 + 4
    return torch.cat([ctr - wh / 2, ctr + wh / 2], dim=1).cuda(), torch.rand(R, generator=g).cuda()


def _nms(R, be):
    boxes, scores = _boxes(R, R)
    return lambda be: (be.nms(boxes, scores, 0.5), be.nms(boxes, scores, 0.3, max_keep=5))


for _R in (1, 63, 64, 65, 300):          # around the 64-box words of the suppression mask
    add("nms-%d" % _R, [Q("nms")], functools.partial(_nms, _R))


def _nms_batched(be):
    counts = [300, 64, 1]
    Rmax = max(counts)
    bs = torch.zeros((3, Rmax, 4), dtype=torch.float32, device="cuda")
    for b, R in enumerate(counts):
        boxes, scores = _boxes(R, 100 + b)
        bs[b, :R] = boxes[torch.argsort(scores, descending=True, stable=True)]
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    live = torch.arange(Rmax, device="cuda")[None, :] < cnt[:, None]           # (flags behind a set's count are not the entry's to write)

    def op(be):
        return (be.nms_batched(bs, cnt, 0.5) & live, be.nms_batched(bs, cnt, 0.3, max_keep=5) & live)
    return op


add("nms-batched-3", [Q("nms_batched")], _nms_batched)


# ---------------------------------------------------------------------------------------------------------------- whole fits
# The net under everything above: whatever route a fit takes at these shapes, its alphas and scores are the same bits with
# every workspace at its reported size and poisoned.  (777, 129, 36) under the shipped storage rule, (1501, 257, 70) compact.
FIT_SHAPES = [("777x129x36-auto", 777, 129, 36, dict(knm_storage="auto")), ("1501x257x70-u24", 1501, 257, 70, dict(knm_storage="u24"))]
LAMS = [1e-3, 1e-4, 1e-5]
MAXITER = 10


def _fit(which, n, M, D, be):
    import odx
    F, Zf, y, X, idx = problem(be, n, M, D)

    def op(be):
        if which == "fit":
            alpha = odx.falkon_fit(be, F, y, Zf, SIGMA, LAM, MAXITER)
            return (alpha, be.mmv(F, Zf, SIGMA, alpha))
        if which == "path":
            alphas = odx.falkon_fit_path(be, F, y, Zf, SIGMA, LAMS, MAXITER)
            return (alphas, be.mmv(F, Zf, SIGMA, alphas.t().contiguous()))
        if which == "multi":
            Y = torch.stack([y, -y, y * (torch.arange(n, device="cuda") % 2).double()], dim=1)
            return (odx.falkon_fit_multi(be, F, Y, Zf, SIGMA, LAM, MAXITER),)
        if which == "cv":
            return tuple(odx.falkon_fit_cv(be, F, y, Zf, SIGMA, LAMS, odx.cv_folds(n, 3, seed=1), 3, MAXITER))
        from odx.wrappers import CenterSelector
        est = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=SIGMA), penalty=LAM, M=M, maxiter=MAXITER,
                               center_selection=CenterSelector(idx), options=odx.FalkonOptions())
        grid = est.fit_grid(X, y, [8.0, 12.0], [1e-3, 1e-5])
        path = est.fit_path(X, y, LAMS)
        one = est.fit(X, y)
        return tuple(e.alpha_ for row in grid for e in row) + tuple(e.alpha_ for e in path) + (one.alpha_, one.predict(X), odx.predict_path(path, X))
    return op


_FIT_QUERIES = {"fit": [Q("falkon_precond")], "path": [Q("falkon_precond_path")], "multi": [Q("falkon_precond")], "cv": [Q("falkon_precond_path")],
                "estimator": [Q("falkon_precond"), Q("falkon_precond_path")]}
for _tag, _n, _M, _D, _set in FIT_SHAPES:
    for _which in ("fit", "path", "multi", "cv", "estimator"):
        add("whole-%s-%s" % (_which, _tag), _FIT_QUERIES[_which], functools.partial(_fit, _which, _n, _M, _D), **_set)


def _job(n, M, D, be):
    """A LockstepClassJob over 3 classes, two per class-batched chain: its factors' workspace ("precond_group") comes through
    _workspace, on the chains' side stream."""
    from odx.job import LockstepClassJob
    X, y = _blob(n, D)
    rng = np.random.default_rng(n)
    cidx = [torch.from_numpy(np.sort(rng.choice(n, M, replace=False)).astype(np.int64)).cuda() for _ in range(3)]
    ys = [y, -y, y * (torch.arange(n, device="cuda") % 3 - 1).double()]

    def op(be):
        alphas = {}
        job = LockstepClassJob(be, X, n, M, lambda c: ys[c], cidx, SIGMA, LAM, MAXITER, _solver_options(), precond_batch=2)
        job.run(be.features(X), [0, 1, 2], alphas_out=alphas)
        torch.cuda.synchronize()
        res = tuple(alphas[c].clone() for c in range(3)) + (job.scores.clone(),)
        job.release()
        return res
    return op


add("whole-job-1501x257x70-u24", [Q("falkon_precond_batched")], functools.partial(_job, 1501, 257, 70), knm_storage="u24")


# ---------------------------------------------------------------------------------------------------------------- the table
COVERS = {}
for _cid, _case in CASES.items():
    for _q in _case.queries:
        COVERS.setdefault(_q, []).append(_cid)


@pytest.mark.parametrize("cid", list(CASES))
def test_workspace_contract(be, cid):
    run_case(be, CASES[cid])


# ---------------------------------------------------------------------------------------------------------------- the promised alignment
# include/odx.h promises 16-byte aligned workspaces where it says anything, and the allocator hands out 512: here the slice
# starts at 16 bytes past a 512-byte boundary.  The whole fits and one case per family and layout; every entry was read first
# (docs/workspace_contract.md has the reading, entry by entry): none derives anything from the workspace's address beyond 16
# bytes, and every sub-buffer an entry cuts from its workspace starts at a multiple of 16 bytes from its beginning.
OFFSET16_CASES = [cid for cid in CASES if cid.startswith("whole-")] + [
    "build-f32-t128-513x257x70", "build-u24-t256-513x257x70", "build-m32-f32-513x257x70", "build-rows-bf16-f32-513x257x70",
    "build-sigmas-u24-513x257x70",
    "score-ranges-gauss-t128-513x1300x9", "score-dense-gauss-t256-513x1300x9", "score-sigmas-gauss-t0-513x1300x9",
    "score-dense-f8-t0-513x1300x9", "score-ranges-rowsbf16-t256-513x1300x9", "score-dense-rowsf16-t128-513x1300x9",
    "score-dense-m52-t0-513x1300x9", "score-short-ranges-gauss-t256",
    "pass12-f32-5085", "pass12-u24-5085", "pass12-bf16-20440", "pass12-mapped-u24-5085",
    "passn-u24-2524-nv11", "passn-bf16-5084-nv5", "passn-u24-20440-nv11",
    "stream-own-ring-300x64-ragged", "stream-small-ring-300x64-ragged",
    "precond-gauss-257", "precond-m52-130", "precond-gauss-4100-split", "precond-batched-ragged", "precond-batched-partial-t-inverse",
    "precond-path-gauss-257", "tri-blocked-mv-1000", "potrf-trtri-300",
    "cg-solve-777x129", "cg-batched-f32", "cg-batched-u24", "cg-batched-bf16",
    "rls-single-D64", "rls-single-D70", "rls-batched-D64", "rls-batched-D70",
    "nms-300", "nms-batched-3",
]
assert set(OFFSET16_CASES) <= set(CASES), sorted(set(OFFSET16_CASES) - set(CASES))


@pytest.mark.parametrize("cid", OFFSET16_CASES)
def test_workspace_at_the_promised_alignment(be, cid):
    run_case(be, CASES[cid], offset16=True)
