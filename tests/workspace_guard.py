"""Hold every workspace of a backend to exactly the size its call site asked for, between two guard bands, filled with a
poison byte (a plain helper module: tests/test_workspace_guard_host.py tests it on the CPU, tests/test_gpu_workspace_contract.py
uses it on the GPU).

HipBackend._workspace(key, nbytes) keeps one buffer per key and only ever grows it, torch rounds every allocation up, and
the buffer carries the previous call's finite numbers: a *_workspace_bytes twin that reports too little, a call site that
asks the wrong twin, a slab row written past the end, and a slab cell read before anybody wrote it in this call all leave
the results right.  `guarded(be, poison)` replaces be._workspace, on the instance and for the duration of the context, by
one that

  * defers to the original while a HIP graph is being captured (graph-owned buffers must stay as they are);
  * otherwise never reuses a buffer: each request gets GUARD + max(nbytes, 16) + GUARD fresh bytes, ALL of them set to
    `poison`, and the middle slice is handed out — its numel() is what the original guarantees at least, and since the
    backend passes ws.numel() as workspace_bytes, every entry's own size check runs at exactly the reported size;
  * records (key, nbytes, buffer) and keeps the buffers alive until check().

check() synchronises and asserts that both bands of every buffer still hold `poison` everywhere.

The three constants, and why:
  GUARD = 65536   a multiple of 256, so the slice keeps the allocator's alignment (only the size changes, not the
                  alignment the kernels have always run at); and wide enough that a slab row written one leading
                  dimension too far still lands inside the band at the test shapes (the widest slab row there is
                  round_up(20440, 4) doubles = 163 520 B for the few M = 20440 cases, 8 * 2048 = 16 KiB and less
                  everywhere else: a row that starts less than GUARD past the end is caught from its first byte on).
  0xFF            every f64, f32, bf16 and f16 cell of the workspace is a NaN and every integer -1: a cell that is read
                  before it is written turns the result into NaN (or an index into -1).
  0x5A            every cell is finite, huge garbage (f64 0x5A5A.. = 2.9e130, f32 1.5e16), a different value from the other
                  poison and from zero: a stale read that a NaN would not show (a max, a compare, an integer count) gives
                  two different results under the two poisons.
"""
import contextlib
import re

import torch

GUARD = 65536
POISON_NAN = 0xFF
POISON_FINITE = 0x5A
POISONS = (POISON_NAN, POISON_FINITE)
OFFSET = 16            # offset16=True: the slice starts 16 bytes further in — the alignment include/odx.h promises, no more

_QUERY = re.compile(r"^odx_\w+_workspace_bytes$")


def header_queries(text):
    """The names of the *_workspace_bytes twins that a header text declares (or mentions with a call's parenthesis)."""
    return set(re.findall(r"(odx_\w+_workspace_bytes)\(", text))


class Guard:
    """What `guarded` yields: the record of the workspaces handed out and of the queries asked."""

    def __init__(self, poison, offset16=False):
        if not 0 <= int(poison) <= 255:
            raise ValueError("poison must be one byte")
        self.poison = int(poison)
        self.shift = OFFSET if offset16 else 0
        self.records = []           # (key, nbytes, whole buffer)
        self.queries = []           # (name, args)

    def allocate(self, key, nbytes, device):
        nbytes = max(int(nbytes), 16)
        buf = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        buf.fill_(self.poison)
        self.records.append((key, nbytes, buf))
        lo = GUARD + self.shift
        return buf[lo:lo + nbytes]

    def asked(self):
        """The set of the *_workspace_bytes names that were called inside the context."""
        return {name for name, _ in self.queries}

    def keys(self):
        return [key for key, _, _ in self.records]

    def check(self):
        """Both guard bands of every buffer still hold the poison.  Offsets in the message are relative to the END of the
        slice (negative ones below -nbytes lie in the band before it)."""
        for _, _, buf in self.records:
            if buf.is_cuda:
                torch.cuda.synchronize(buf.device)
                break
        for key, nbytes, buf in self.records:
            end = GUARD + self.shift + nbytes
            before, after = buf[:end - nbytes] != self.poison, buf[end:] != self.poison
            if bool(before.any()) or bool(after.any()):
                at = torch.cat([torch.nonzero(before).view(-1) - end, torch.nonzero(after).view(-1)])
                first, last = int(at[0]), int(at[-1])
                side = "before the slice" if last < 0 else "after the slice" if first >= 0 else "on both sides of the slice"
                raise AssertionError("workspace %r of %d bytes: %d guard bytes overwritten %s, offsets %+d .. %+d from the end of the slice"
                                     % (key, nbytes, int(at.numel()), side, first, last))
        self.records = []


def _recorded(guard, name, fn):
    def query(*args):
        guard.queries.append((name, args))
        return fn(*args)
    return query


@contextlib.contextmanager
def guarded(be, poison, offset16=False):
    """See the module's docstring.  Yields the Guard; be._workspace and the *_workspace_bytes attributes of be.lib are as
    they were afterwards, also when the body raises.  check() is the caller's to call (inside or after the context)."""
    guard = Guard(poison, offset16)
    original = be._workspace
    had_own = "_workspace" in vars(be)

    def workspace(key, nbytes):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return original(key, nbytes)
        return guard.allocate(key, nbytes, be.device)

    lib = be.lib
    # (a ctypes CDLL keeps every symbol it has bound as a plain instance attribute, and odx.hip.load() binds them all:
    # setattr and restoring is all it takes)
    saved = {nm: fn for nm, fn in vars(lib).items() if _QUERY.match(nm)}
    be._workspace = workspace
    for nm, fn in saved.items():
        setattr(lib, nm, _recorded(guard, nm, fn))
    try:
        yield guard
    finally:
        for nm, fn in saved.items():
            setattr(lib, nm, fn)
        if had_own:
            be._workspace = original
        else:
            del be._workspace

