"""The host side of the partial inverse of T, without a GPU: the one rule for who gets one (odx.job.t_inverse_stop), the
Precond slot that carries the block boundaries, HipBackend.trmv's dispatch on it (against recorded library calls), and the refusal
of every other consumer of a Precond."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


def test_rule_only_above_8192_centres_and_only_levels_of_4096_rows_and_more():
    from odx.job import t_inverse_stop
    for M in (1, 128, 600, 4096, 4097, 8191, 8192):
        for u in (0, 1, 2):
            assert t_inverse_stop(M, u) == 0, (M, u)
    for M in (8193, 10000, 16384):                              # top level 8192
        assert [t_inverse_stop(M, u) for u in (0, 1, 2)] == [0, 8192, 4096], M
    for M in (16385, 20000, 32768):                             # top level 16384
        assert [t_inverse_stop(M, u) for u in (0, 1, 2)] == [0, 16384, 8192], M
    # the test hook: that level wherever rows lie beyond it, whatever the option says
    assert t_inverse_stop(600, 0, 256) == 256 and t_inverse_stop(256, 2, 256) == 0 and t_inverse_stop(10000, 1, 256) == 256


class _Lib:
    """Records what HipBackend hands the library."""

    def __init__(self, options=None):
        self.calls, self.options = [], dict(options or {})

    def odx_get_option(self, name, ref):
        ref._obj.value = self.options[name.decode()]
        return 0

    def odx_tri_blocked_mv_workspace_bytes(self, M):
        return 16 * ((M + 1) // 2)

    def odx_tri_blocked_mv_f64(self, *a):
        self.calls.append(("blocked",) + a)
        return 0

    def odx_trmv_f64(self, *a):
        self.calls.append(("merged",) + a)
        return 0


def _backend():
    from odx.backend import HipBackend
    be = HipBackend.__new__(HipBackend)
    be.lib, be.device = _Lib(), torch.device("cpu")
    be._workspace = lambda key, nbytes: torch.zeros(max(int(nbytes), 16), dtype=torch.uint8)
    be._stream = lambda: ctypes.c_void_p(0)
    return be


def _precond(M, blocks=()):
    from odx.backend import Precond
    P = Precond()
    assert P.blocks == ()                                       # the slot exists on every Precond and starts empty
    P.M, P.ld = M, (M + 1) // 2 * 2
    P.LTi, P.LTit, P.LAi, P.LAit = (torch.zeros((M, P.ld), dtype=torch.float64) for _ in range(4))
    P.blocks = tuple(blocks)
    return P


def test_trmv_dispatches_on_the_block_boundaries():
    be = _backend()
    x, z, out = (torch.zeros(10, dtype=torch.float64) for _ in range(3))
    P = _precond(10, (0, 4, 8, 10))
    for name in ("LTi", "LTit", "LAi", "LAit"):
        be.trmv(P, name, x, alpha=0.5, beta=2.0, z=z, out=out)
    kinds = [c[0] for c in be.lib.calls]
    assert kinds == ["blocked", "blocked", "merged", "merged"]              # A's factors are whole inverses either way
    for call, name, uplo in zip(be.lib.calls, ("LTi", "LTit"), (0, 1)):
        _, tri, ld, M, up, bounds, nblocks, xp, alpha, beta, zp, yp, ws, ws_bytes, _stream = call
        assert tri.value == getattr(P, name).data_ptr() and (ld, M, up, nblocks) == (10, 10, uplo, 3)
        assert list(bounds) == [0, 4, 8, 10] and (alpha, beta) == (0.5, 2.0)
        assert (xp.value, zp.value, yp.value) == (x.data_ptr(), z.data_ptr(), out.data_ptr())
        assert ws_bytes >= be.lib.odx_tri_blocked_mv_workspace_bytes(10)
    be.lib.calls.clear()
    for name in ("LTi", "LTit"):
        be.trmv(_precond(10), name, x, out=out)
    assert [c[0] for c in be.lib.calls] == ["merged", "merged"]             # an empty slot: today's one launch


def test_every_other_consumer_refuses_a_partial_factor():
    from odx.backend import Knm, require_merged
    be = _backend()
    P = _precond(10, (0, 4, 10))
    require_merged(_precond(10), "anything")
    K = Knm()
    K.n, K.M, K.ld, K.K = 4, 10, 12, torch.zeros((4, 12))
    with pytest.raises(ValueError, match="partial inverse"):
        be.cg_solve(K, P, torch.zeros(10, dtype=torch.float64), 4, 1e-5, 3, None)
    with pytest.raises(ValueError, match="partial inverse"):
        be.cg_solve_batched([K], [P], torch.zeros((1, 10), dtype=torch.float64), [4], 1e-5, 3, None)
    with pytest.raises(ValueError, match="partial inverse"):
        be.trmvn(P, "LTi", torch.zeros((2, 10), dtype=torch.float64))
    assert be.lib.calls == []


def test_job_reads_the_rule_from_the_librarys_options():
    from odx.job import LockstepClassJob

    class _Be:
        pass

    job = LockstepClassJob.__new__(LockstepClassJob)
    job.be, job.M = _Be(), 10000
    assert job._t_stop() == 0                                               # a backend without the library (the tests' oracle backend)
    job.be.lib = _Lib({"t_inverse_unmerged": 0, "t_inverse_force_stop": 0})
    assert job._t_stop() == 0
    job.be.lib.options["t_inverse_unmerged"] = 2
    assert job._t_stop() == 4096
    job.M = 8192
    assert job._t_stop() == 0
    job.be.lib.options["t_inverse_force_stop"] = 256
    assert job._t_stop() == 256


def test_library_options_of_the_partial_inverse():
    from odx import hip
    lib = ctypes.CDLL(hip.lib_path())
    got = ctypes.c_int(-99)
    assert lib.odx_option_default(b"t_inverse_unmerged", ctypes.byref(got)) == 0 and got.value in (0, 1, 2)
    default = got.value
    assert lib.odx_get_option(b"t_inverse_unmerged", ctypes.byref(got)) == 0 and got.value == default      # untouched: the default
    assert lib.odx_get_option(b"t_inverse_force_stop", ctypes.byref(got)) == 0 and got.value == 0           # the hook is off
    assert lib.odx_set_option(b"t_inverse_unmerged", 3) != 0
