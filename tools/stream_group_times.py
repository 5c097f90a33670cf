#!/usr/bin/env python3
"""Per-chunk time of the pass kernels of a streamed multi-vector pass (odx_gauss_ktk_stream_h2n) by their position behind the
chunk's build, from the rocpd database of a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o x -- python tools/time_stream_pass.py --n 1e6 --D 1024 --M 1e4 --nv 8
    python tools/stream_group_times.py OUT/x_results.db
A chunk is built once (gauss_knm_h2w256_kernel) and read once per group of vectors.  Later groups markedly slower than the first
would mean the chunk is being evicted from the Infinity Cache between its reads.  Chunks with one pass kernel are the
composition measured beside it (ktk2 / ktk: one build per call)."""
import collections
import json
import sqlite3
import statistics
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    chunks, cur = [], None
    for name, start, end in rows:
        if "gauss_knm_h2w256_kernel" in name:
            cur = []
            chunks.append((end - start, cur))
        elif cur is not None and ("knm_passq" in name or "knm_passnv" in name):
            cur.append(end - start)
    by_groups = collections.defaultdict(list)
    for build, passes in chunks:
        by_groups[len(passes)].append((build, passes))
    for groups in sorted(by_groups):
        if groups == 0:
            continue
        items = by_groups[groups]
        line = {"groups_per_chunk": groups, "chunks": len(items), "build_us_median": statistics.median(b for b, _ in items) / 1e3}
        for g in range(groups):
            d = sorted(p[g] for _, p in items)
            line["group%d_us" % g] = {"median": d[len(d) // 2] / 1e3, "mean": statistics.mean(d) / 1e3, "p90": d[int(len(d) * 0.9)] / 1e3}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
