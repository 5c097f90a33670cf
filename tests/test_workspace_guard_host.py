"""The workspace hook of tests/workspace_guard.py on the CPU — a fake backend whose entries misbehave in the ways the hook
exists to catch — and the coverage table: every *_workspace_bytes twin that include/odx.h declares has a case in
tests/test_gpu_workspace_contract.py (COVERS), so an entry with a workspace cannot be added without one."""
import os
import re
import types

import pytest

torch = pytest.importorskip("torch")

from tests import workspace_guard as wg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeBackend:
    """_workspace as HipBackend has it (one buffer per key, only ever grown), device "cpu", and a lib of two queries."""

    def __init__(self):
        self.device = "cpu"
        self._ws = {}
        self.lib = types.SimpleNamespace(odx_fake_workspace_bytes=lambda n: 8 * n, odx_other_workspace_bytes=lambda n, m: n * m,
                                         odx_fake=lambda *a: 0)

    def _workspace(self, key, nbytes):
        nbytes = max(int(nbytes), 16)
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._ws[key] = torch.zeros(nbytes, dtype=torch.uint8)
        return buf

    # ---- entries
    def good(self, n):
        ws = self._workspace("good", self.lib.odx_fake_workspace_bytes(n))
        ws[:8 * n].view(torch.float64).copy_(torch.arange(n, dtype=torch.float64))
        return ws[:8 * n].view(torch.float64).sum()

    def writes_before(self, n):
        ws = self._workspace("under", self.lib.odx_fake_workspace_bytes(n))
        ws._base[ws.storage_offset() - 1] = 7
        return ws

    def writes_after(self, n, past=0):
        ws = self._workspace("over", self.lib.odx_fake_workspace_bytes(n))
        ws._base[ws.storage_offset() + ws.numel() + past] = 7
        return ws

    def sums_everything(self, n):
        """Reads cells nobody wrote in this call."""
        ws = self._workspace("stale", self.lib.odx_fake_workspace_bytes(n))
        return ws.to(torch.int64).sum()


def test_a_well_behaved_entry_passes_and_sees_exactly_the_reported_size():
    be = FakeBackend()
    plain = be.good(5)
    for poison in wg.POISONS:
        with wg.guarded(be, poison) as g:
            assert torch.equal(be.good(5), plain)
            ws = be._workspace("probe", 40)
            assert ws.numel() == 40 and bool((ws == poison).all()) and ws.data_ptr() % 16 == 0
            assert be._workspace("tiny", 0).numel() == 16          # what the original guarantees at least
            assert be._workspace("probe", 40).data_ptr() != ws.data_ptr(), "a buffer was reused"
            g.check()
        assert g.asked() == {"odx_fake_workspace_bytes"} and g.queries[0] == ("odx_fake_workspace_bytes", (5,))


def test_one_byte_before_the_slice_fails_with_key_and_offset():
    be = FakeBackend()
    with wg.guarded(be, 0xFF) as g:
        be.writes_before(4)
        with pytest.raises(AssertionError) as e:
            g.check()
    msg = str(e.value)
    assert "'under'" in msg and "32 bytes" in msg and "before the slice" in msg and "offsets -33 .. -33" in msg, msg


@pytest.mark.parametrize("past", [0, 300, wg.GUARD - 1])
def test_one_byte_after_the_slice_fails_with_key_and_offset(past):
    be = FakeBackend()
    with wg.guarded(be, 0x5A) as g:
        be.good(3)
        be.writes_after(4, past)
        with pytest.raises(AssertionError) as e:
            g.check()
    msg = str(e.value)
    assert "'over'" in msg and "32 bytes" in msg and "after the slice" in msg and "offsets +%d .. +%d" % (past, past) in msg, msg


def test_a_stale_read_gives_different_results_under_the_two_poisons():
    be = FakeBackend()
    got = []
    for poison in wg.POISONS:
        with wg.guarded(be, poison) as g:
            got.append(int(be.sums_everything(4)))
            g.check()                                             # (it wrote nowhere: the bands are intact)
    assert got[0] != got[1] and got == [32 * 0xFF, 32 * 0x5A]
    assert int(be.sums_everything(4)) == 0                        # the recycled buffer of the plain run hides it


def test_offset16_moves_the_slice_by_sixteen_bytes_and_keeps_the_bands():
    be = FakeBackend()
    with wg.guarded(be, 0xFF, offset16=True) as g:
        ws = be._workspace("k", 48)
        assert ws.numel() == 48 and ws.storage_offset() == wg.GUARD + 16
        assert ws.data_ptr() % 16 == 0 and (ws.data_ptr() - 16) % 64 == 0 and ws.data_ptr() % 32 != 0
        ws._base[ws.storage_offset() - 1] = 0                     # the 16 bytes in front of it belong to the band
        with pytest.raises(AssertionError, match="before the slice"):
            g.check()


def test_everything_is_restored_also_when_the_body_raises():
    be = FakeBackend()
    q0, q1, f = be.lib.odx_fake_workspace_bytes, be.lib.odx_other_workspace_bytes, be.lib.odx_fake
    assert "_workspace" not in vars(be)
    with pytest.raises(RuntimeError, match="boom"):
        with wg.guarded(be, 0xFF):
            assert be.lib.odx_fake_workspace_bytes is not q0 and be.lib.odx_fake is f
            assert "_workspace" in vars(be)
            raise RuntimeError("boom")
    assert be.lib.odx_fake_workspace_bytes is q0 and be.lib.odx_other_workspace_bytes is q1 and be.lib.odx_fake is f
    assert "_workspace" not in vars(be) and be._workspace.__func__ is FakeBackend._workspace
    # an instance that had its own _workspace gets that one back
    own = be._workspace
    be._workspace = own
    with wg.guarded(be, 0x5A):
        pass
    assert vars(be)["_workspace"] is own


def test_the_guard_is_a_multiple_of_256_and_the_poisons_are_what_the_docstring_says():
    import struct
    assert wg.GUARD % 256 == 0
    nan64, = struct.unpack("<d", bytes([wg.POISON_NAN]) * 8)
    nan32, = struct.unpack("<f", bytes([wg.POISON_NAN]) * 4)
    assert nan64 != nan64 and nan32 != nan32
    assert struct.unpack("<i", bytes([wg.POISON_NAN]) * 4)[0] == -1
    for dt in (torch.bfloat16, torch.float16):
        assert bool(torch.isnan(torch.tensor([wg.POISON_NAN] * 2, dtype=torch.uint8).view(dt)).all())
    big64, = struct.unpack("<d", bytes([wg.POISON_FINITE]) * 8)
    big32, = struct.unpack("<f", bytes([wg.POISON_FINITE]) * 4)
    assert 1e100 < big64 < float("inf") and 1e15 < big32 < float("inf")


def test_every_workspace_query_of_the_header_has_a_case():
    """include/odx.h <-> COVERS: the same set of names, every name with at least one case id, every id a case that exists
    (or, for an entry held elsewhere, the name of an existing test: none at present)."""
    from tests import test_gpu_workspace_contract as gpu
    with open(os.path.join(ROOT, "include", "odx.h")) as f:
        text = f.read()
    declared = set(re.findall(r"(odx_\w+_workspace_bytes)\(", text))
    assert declared == wg.header_queries(text) and declared
    assert declared == set(gpu.COVERS), (sorted(declared - set(gpu.COVERS)), sorted(set(gpu.COVERS) - declared))
    ids = set(gpu.CASES)
    for name, cases in gpu.COVERS.items():
        assert cases, name
        assert set(cases) <= ids, (name, sorted(set(cases) - ids))
    # and the other way round: what a case claims is a query of the header
    for cid, case in gpu.CASES.items():
        assert set(case.queries) <= declared, cid
