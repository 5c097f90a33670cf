"""The group arithmetic of HipBackend.ktkn above the LDS limit of the one-read pass (odx/knm_path.py: _ktkn_plan /
ktkn_reads), on a stub without a device: which vectors take the two-read route (odx_knm_fwdn_q + odx_knm_bwdn_q), which keep
the one-read groups, pairs and singles, and how many reads of the block that makes."""
import pytest

from odx.knm_path import PathOps


class _Block:
    fmt = "u24"


class _Stub(PathOps):
    """PathOps with the two facts of a block the plan depends on given, not asked of the library."""

    def __init__(self, width, pairs, wide_pass_min):
        self._width, self._pairs, self.wide_pass_min = width, pairs, wide_pass_min

    def ktkn_width(self, K):
        return self._width

    def can_ktk2(self, K):
        return self._pairs


def _reads_of_groups(L, width, pairs):
    """Reads of the one-read grouping: whole groups of `width`, then the remainder as one group."""
    full, rem = divmod(L, width)
    one = lambda g: 1 if g >= 3 or g == 1 or (g == 2 and pairs) else g      # noqa: E731
    return full * one(width) + (one(rem) if rem else 0)


@pytest.mark.parametrize("L", range(1, 18))
@pytest.mark.parametrize("width", [8, 4])
@pytest.mark.parametrize("wmin", [None, 3, 5])
def test_widths_with_a_one_read_pass_never_take_the_route(L, width, wmin):
    be = _Stub(width, True, wmin)
    plan = be._ktkn_plan(_Block(), L)
    assert all(kind != "wide" for kind, _, _ in plan)
    assert [l for _, l, _ in plan] == list(range(0, L, width)) and sum(g for _, _, g in plan) == L
    assert be.ktkn_reads(_Block(), L) == _reads_of_groups(L, width, True)
    for kind, _, g in plan:
        assert kind == ("nv" if g >= 3 else "pair" if g == 2 else "single")


@pytest.mark.parametrize("L", range(1, 18))
@pytest.mark.parametrize("width,pairs", [(2, True), (1, False)])
def test_route_off_is_pairs_and_singles(L, width, pairs):
    be = _Stub(width, pairs, None)
    plan = be._ktkn_plan(_Block(), L)
    assert all(kind == ("pair" if g == 2 else "single") for kind, _, g in plan)
    assert be.ktkn_reads(_Block(), L) == (-(-L // 2) if pairs else L)


@pytest.mark.parametrize("L", range(1, 18))
@pytest.mark.parametrize("width,pairs", [(2, True), (1, False)])
@pytest.mark.parametrize("wmin", [3, 4, 6, 8])
def test_route_on_chunks_of_eight_and_a_remainder_below_the_minimum(L, width, pairs, wmin):
    be = _Stub(width, pairs, wmin)
    plan = be._ktkn_plan(_Block(), L)
    # every vector exactly once, in order
    pos = 0
    for _, l, g in plan:
        assert l == pos and g >= 1
        pos += g
    assert pos == L
    wide = [(l, g) for kind, l, g in plan if kind == "wide"]
    rest = [(kind, g) for kind, _, g in plan if kind != "wide"]
    # chunks of up to 8 while at least wmin vectors remain; what is left below wmin keeps the pairs and singles
    want, left = [], L
    while left >= wmin:
        want.append(min(8, left))
        left -= want[-1]
    assert [g for _, g in wide] == want and sum(g for _, g in rest) == left < wmin
    assert all(kind == ("pair" if g == 2 and pairs else "single") and g <= width for kind, g in rest)
    assert be.ktkn_reads(_Block(), L) == 2 * len(want) + (-(-left // 2) if pairs else left)


def test_the_figures_of_the_headline_width():
    """8 states at M = 1e4 (one read serves two): 4 reads by pairs, 2 through the route; 11 = 8 + 3 -> 4 reads, 10 = 8 + a pair -> 3."""
    on, off = _Stub(2, True, 3), _Stub(2, True, None)
    assert off.ktkn_reads(_Block(), 8) == 4 and on.ktkn_reads(_Block(), 8) == 2
    assert on.ktkn_reads(_Block(), 11) == 4 and on.ktkn_reads(_Block(), 10) == 3 and on.ktkn_reads(_Block(), 2) == 1
    assert _Stub(8, False, 3).ktkn_reads(_Block(), 8) == 1 and _Stub(4, True, 3).ktkn_reads(_Block(), 8) == 2


def test_f32_blocks_never_take_the_route():
    class F32:
        fmt = "f32"
    be = _Stub(2, True, 3)
    assert all(kind != "wide" for kind, _, _ in be._ktkn_plan(F32(), 8)) and be.ktkn_reads(F32(), 8) == 4
