"""The column map of a centre list that names some centres more than once.

The reference's centre rule draws with replacement, so some columns of a class's K_nM block are copies of others.  A block
built on the DISTINCT centres only (in order of first occurrence: a column subsequence of the full block) has fewer columns
to build and to stream, while every M-vector of the fit keeps its length and meaning: with ``col_of[j]`` the distinct column
of list position j,

    K_full v = K_d fold(v),   fold(v)[d] = sum of v[j] over col_of[j] = d,        (K_full' t)[j] = (K_d' t)[col_of[j]].

``column_map`` is host arithmetic on the index vector (made once per class, outside every step); the kernels read the map
as three int32 vectors (include/odx.h, "Distinct columns").
"""
import torch


class ColumnMap:
    """Mv list positions over Md distinct columns.  first (Md,) int64: the list position a column first occurs at, ascending;
    col_of (Mv,) int32; start (Md + 1,) / pos (Mv,) int32: the positions of column d are pos[start[d]:start[d + 1]],
    ascending.  Host tensors; ``on(device)`` hands out (and keeps) their copies on a device."""
    __slots__ = ("Mv", "Md", "first", "col_of", "start", "pos", "_dev")

    def __init__(self, Mv, first, col_of, start, pos):
        self.Mv, self.Md = int(Mv), int(first.numel())
        self.first, self.col_of, self.start, self.pos = first, col_of, start, pos
        self._dev = {}

    def on(self, device):
        """(first, col_of, start, pos) on `device`.  The first call per device copies them there: call it where a wait for
        the copy does no harm (LockstepClassJob does, in its constructor)."""
        key = str(torch.device(device))
        got = self._dev.get(key)
        if got is None:
            got = self._dev[key] = tuple(t.to(device) for t in (self.first, self.col_of, self.start, self.pos))
        return got

    def fold(self, v):
        """fold(v) with torch arithmetic on v's device, left to right per column (tests, host-side checks)."""
        out = torch.zeros(self.Md, dtype=v.dtype, device=v.device)
        pos = self.pos.to(v.device).long()
        start = self.start.tolist()
        most = max(b - a for a, b in zip(start[:-1], start[1:]))
        first_of = torch.as_tensor(start[:-1], device=v.device)
        count = torch.as_tensor(start[1:], device=v.device) - first_of
        for k in range(most):                     # k-th occurrence of every column that has one
            has = count > k
            out[has] = out[has] + v[pos[first_of[has] + k]]
        return out

    def expand(self, x):
        """x over the distinct columns -> the Mv list positions."""
        return x[self.col_of.to(x.device).long()]


def column_map(idx):
    """The ColumnMap of the centre index vector `idx` (M,), or None when no centre occurs twice."""
    ih = torch.as_tensor(idx).detach().cpu().to(torch.int64).reshape(-1)
    M = ih.numel()
    if M >= 2 ** 31:
        raise ValueError("column_map: %d positions do not fit the map's int32 indices" % M)
    uniq, inv = torch.unique(ih, return_inverse=True)           # sorted values; inv[j] = the value's place among them
    Md = uniq.numel()
    if Md == M:
        return None
    at = torch.arange(M, dtype=torch.int64)
    first_of_value = torch.full((Md,), M, dtype=torch.int64).scatter_reduce_(0, inv, at, "amin")
    order = torch.argsort(first_of_value)                       # distinct column d = the value first seen d-th
    rank = torch.empty(Md, dtype=torch.int64)
    rank[order] = torch.arange(Md, dtype=torch.int64)
    col_of = rank[inv]
    pos = torch.argsort(col_of, stable=True)                    # grouped by column, list order inside
    start = torch.zeros(Md + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(torch.bincount(col_of, minlength=Md), 0)
    return ColumnMap(M, first_of_value[order].contiguous(), col_of.to(torch.int32), start.to(torch.int32), pos.to(torch.int32))
