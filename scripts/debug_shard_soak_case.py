#!/usr/bin/env python3
"""Replays one case of the shard soak (tests/test_gpu_shard_soak.py) and prints every comparison that differs: the plan
and its cuts, the request or the episodes' rule, the operator, the combination (folded, folded backwards, chained) and
what the operator's own rule said (debug tool).
Usage: debug_shard_soak_case.py INDEX [seams|anywhere] [operator, e.g. sample_at or m4_buckets]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb, linked_soak as ls, shard_soak as ss, test_gpu_shard_soak as t  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402

_abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = True   # (the slice switches are set per case, as under pytest)
index = int(sys.argv[1])
plans = [name for name in sys.argv[2:] if name in ss.PLANS] or list(ss.PLANS)
operators = [name for name in sys.argv[2:] if name not in ss.PLANS]
unknown = [name for name in operators if not any(name in names for names in t.OPERATORS.values())]
if unknown:
    sys.exit(f"no such plan or operator: {unknown}; operators: {sorted(sum(t.OPERATORS.values(), ()))}")
families = [family for family, names in t.OPERATORS.items() if not operators or set(operators) & set(names)]
planned = t.planned_case(index)
if planned is None:
    print("case", index, "has more than", ls.MAX_ROWS, "rows: the soak leaves it out")
    sys.exit(0)
drawn = planned.drawn
types = np.bincount(drawn.batch.model_type_id, minlength=len(mdb.MODEL_TYPE_NAMES))
print("case", index, "series", drawn.kinds, "grouping", drawn.grouping, "groups", drawn.n_groups, "tail", drawn.n_tail,
      "segments", len(drawn.batch), dict(zip(mdb.MODEL_TYPE_NAMES, types.tolist())), "rows", len(drawn.timestamps),
      "permuted", drawn.permuted, ls.row_census(drawn))
print("filter", drawn.filter_spec, "slices of", drawn.slice_pairs, "pairs,", drawn.slice_points, "points;",
      len(planned.links), "boundaries with a link,", len(planned.linked_seams), "seams,", len(planned.episode_seams),
      "episode seams; the chain starts from", "fresh cells" if index % 2 else "the one call's cells")
for name in plans:
    print(" ", ss.describe(planned.plans[name]), ss.plan_census(planned, planned.plans[name]))
bad = []


def report(where, operator, form, differences):
    if differences:
        bad.append((where, operator, form))
        print(f"{where}\n  {operator} [{form}]: {len(differences)} difference(s)")
        for line in differences[:10]:
            print("    " + line)


context = mdb.Context(0)
ranks = [mdb.Context(0) for _ in range(t.N_CONTEXTS)]
for family in families:
    census = t._new_census()
    t.run_case(context, ranks, index, family, census, plans=plans, operators=operators or None, report=report)
    print(f"{family}: " + ", ".join(f"{count} {name}" for name, count in census.items()))
print("comparisons that differ:", len(bad))
sys.exit(1 if bad else 0)
