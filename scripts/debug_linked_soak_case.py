#!/usr/bin/env python3
"""Replays one case of the linked-row operators' soak (tests/test_gpu_linked_soak.py) and prints every difference: the
request or the episodes' rule, the operator, the form and what the operator's own assertion said (debug tool).
Usage: debug_linked_soak_case.py INDEX [integral|sample|change|episodes]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb, linked_soak as ls, test_gpu_linked_soak as t  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402

_abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = True   # (the slice switches are set per case, as under pytest)
index = int(sys.argv[1])
operators = sys.argv[2:] or list(t.OPERATORS)
drawn = ls.draw(index)
if drawn is None:
    print("case", index, "has more than", ls.MAX_ROWS, "rows: the soak leaves it out")
    sys.exit(0)
types = np.bincount(drawn.batch.model_type_id, minlength=len(mdb.MODEL_TYPE_NAMES))
print("case", index, "series", drawn.kinds, "grouping", drawn.grouping, "groups", drawn.n_groups, "tail", drawn.n_tail,
      "segments", len(drawn.batch), dict(zip(mdb.MODEL_TYPE_NAMES, types.tolist())), "rows", len(drawn.timestamps),
      "permuted", drawn.permuted, ls.row_census(drawn))
print("filter", drawn.filter_spec, "list cuts", drawn.list_cuts, "slices of", drawn.slice_pairs, "pairs,",
      drawn.slice_points, "points")
for request in drawn.sample_requests:
    print("  request", ls.describe(request))
bad = []


def report(where, operator, form, differences):
    if differences:
        bad.append((where, operator, form))
        print(f"{where}\n  {operator} [{form}]: {len(differences)} difference(s)")
        for line in differences[:10]:
            print("    " + line)


context = mdb.Context(0)
for operator in operators:
    census = t._Census()
    t.run_case(context, index, operator, census, report)
    print(f"{operator}: {census.checked} checked numerically, {census.non_finite} only have to be non-finite")
print("comparisons that differ:", len(bad))
sys.exit(1 if bad else 0)
