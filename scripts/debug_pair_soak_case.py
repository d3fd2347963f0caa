#!/usr/bin/env python3
"""Replays one case of the two-field operators' soak (tests/test_gpu_pair_soak.py) and prints every difference: the
request, what was compared and what the operator's own assertion said (debug tool).
Usage: debug_pair_soak_case.py INDEX [one|shards]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb, pair_soak as ps, test_gpu_pair_soak as t  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402

_abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = True   # (as under pytest)
index = int(sys.argv[1])
tiers = sys.argv[2:] or ["one", "shards"]
drawn = ps.draw(index)
if drawn is None:
    print("case", index, "has more than", ps.MAX_ROWS, "rows: the soak leaves it out")
    sys.exit(0)
paths = np.bincount(ps.segment_paths(drawn.x.batch), minlength=len(ps.PATHS))
print("case", index, "y", drawn.kind, "series", drawn.kinds, "grouping", drawn.grouping, "groups", drawn.n_groups, "tail",
      drawn.n_tail, "permuted", drawn.permuted, "rows", len(drawn.x.ts), "segments of x", len(drawn.x.batch),
      dict(zip(ps.PATHS, paths.tolist())), "segments of y", len(drawn.y.batch))
print("edges", len(drawn.edges), "list cuts x", drawn.x_cuts, "y", drawn.y_cuts, "slices of", drawn.slice_pairs,
      "common cut rows", drawn.common_rows)
for request in drawn.requests:
    print("  request", ps.describe(request))
bad = []


def report(where, what, differences):
    if differences:
        bad.append((where, what))
        print(f"{where}\n  {what}: {len(differences)} difference(s)")
        for line in differences[:10]:
            print("    " + line)


context = mdb.Context(0)
for tier in tiers:
    census = t._Census()
    if tier == "one":
        t.run_case(context, index, census, report)
    elif drawn.permuted:
        print("shards: x is permuted, the shard tier leaves the case out")
        continue
    else:
        t.run_shard_case(context, index, census, report)
    census.tell(tier)
print("comparisons that differ:", len(bad))
sys.exit(1 if bad else 0)
