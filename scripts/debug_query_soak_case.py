#!/usr/bin/env python3
"""Replays one case of the query operators' soak (tests/test_gpu_query_soak.py) and prints every difference: the
request, the operator, the form, the cell and the two values (debug tool). Usage: debug_query_soak_case.py INDEX"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb, query_soak as qs, test_gpu_query_soak as t  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402

_abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = True   # (MDB_AGG_BUCKET_SLICE_PAIRS is set per case, as under pytest)
index = int(sys.argv[1])
case = qs.make_case(index)
types = np.bincount(case.batch.model_type_id, minlength=len(mdb.MODEL_TYPE_NAMES))
print("case", index, "series", case.n_groups, case.kinds, "segments", len(case.batch),
      dict(zip(mdb.MODEL_TYPE_NAMES, types.tolist())), "points", len(case.timestamps), "permuted", case.permuted)
print("filter", case.filter_spec, "edges", len(case.edges), "q", case.q, "interpolate", case.interpolate,
      "time range", case.time_range, "list cuts", case.list_cuts, "slices of 1000 pairs", case.slice_pairs)
bad = []


def report(where, operator, form, differences):
    if differences:
        bad.append((where, operator, form))
        print(f"{where}\n  {operator} [{form}]: {len(differences)} difference(s)")
        for line in differences[:10]:
            print("    " + line)


t.run_case(mdb.Context(0), index, report)
print("comparisons that differ:", len(bad))
sys.exit(1 if bad else 0)
