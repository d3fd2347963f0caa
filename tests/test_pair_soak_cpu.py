"""The generator and the references of the two-field operators' soak (tests/pair_soak.py), held to their promises
without a GPU over the default indices of tests/test_gpu_pair_soak.py: draw() is a pure function of its index; the two
grids line up under every request; at most a third of the indices are left out; at most 2 % of the finite cells of
either operator are ill-conditioned under the f64 emulation of the documented rule; the census of what the cases hold
has no empty line; the Python port of the merge rules gives the bytes of mdb.comoments_merge and mdb.moments_merge
(host arithmetic, no GPU); and the two references agree with each other where mdb.h says the operators do."""

import collections

import numpy as np
import pytest

import binned_cases as bc
import comoments_cases as cc
import pair_soak as ps
import modelardb_rs_amd as mdb

N_INDICES = 60   # the default of MDB_PAIR_SOAK_CASES
ILL_CONDITIONED_CAP = 0.02


@pytest.fixture(scope="module")
def drawn_cases():
    return [ps.draw(index) for index in range(N_INDICES)]


@pytest.fixture(scope="module")
def census(drawn_cases):
    """(counts, per operator [ill-conditioned cells, finite cells]) from the references of every drawn case."""
    counts, cells = collections.Counter(), {"comoments": [0, 0], "binned": [0, 0]}
    for drawn in drawn_cases:
        if drawn is None:
            continue
        x, y = drawn.x, drawn.y
        counts["kind " + drawn.kind] += 1
        counts["grouping " + drawn.grouping] += 1
        counts["permuted x"] += drawn.permuted
        counts["tails"] += drawn.n_tail > 0
        counts["list cuts"] += drawn.x_cuts is not None
        counts["slice sizes"] += drawn.slice_pairs is not None
        paths = ps.segment_paths(x.batch)
        for k, name in enumerate(ps.PATHS):
            counts["x segments: " + name] += int((paths == k).sum())
        on_lines = x.values[np.isfinite(x.values) & (x.batch.model_type_id == mdb.MDB_SWING_ID)[x.segment]]
        counts["edges equal to a value on a Swing line"] += int(np.isin(bc.keys_of(drawn.edges), bc.keys_of(on_lines)).sum())
        if not drawn.permuted:   # (rows are the same instants in both fields)
            counts["rows with a NaN in x only"] += int((np.isnan(x.values) & ~np.isnan(y.values)).sum())
            counts["rows with a NaN in y only"] += int((np.isnan(y.values) & ~np.isnan(x.values)).sum())
        counts["rows with +inf in y"] += int((y.values == np.inf).sum())
        counts["rows with -inf in y"] += int((y.values == -np.inf).sum())
        for request in drawn.requests:
            assert request.width >= 1 and 1 <= drawn.n_groups * request.n_buckets <= 2048, drawn.index
            counts["requests"] += 1
            counts["requests of style " + request.style] += 1
            counts["buckets of width 1"] += request.width == 1
            for k in ps.cut_paths(drawn, request):
                counts["t_lo strictly inside an x segment: " + ps.PATHS[k]] += 1
            expected, rule = ps.reference_comoments(drawn, request), ps.rule_cells(drawn, request)
            assert np.array_equal(rule["count"], expected["count"]), drawn.index
            well, plain = ps.well_conditioned_cells(rule, expected)
            cells["comoments"][0] += int((plain & ~well).sum())
            cells["comoments"][1] += int(plain.sum())
            counts["comoments cells with a non-finite point"] += int(((expected["count"] > 0) & ~plain).sum())
            expected, rule = ps.reference_binned(drawn, request), ps.rule_binned(drawn, request)
            assert np.array_equal(rule["count"], expected["count"]), drawn.index
            well, plain = ps.well_conditioned_binned(rule, expected)
            cells["binned"][0] += int((plain & ~well).sum())
            cells["binned"][1] += int(plain.sum())
            counts["binned calls whose keys do not ascend"] += not rule["keys ascend"]
            counts["binned runs"] += expected["runs"]
            counts["binned cells fed by more than one run and more than one segment"] += \
                int(((expected["cell_runs"] > 1) & (expected["segments"] > 1)).sum())
    return counts, cells


def test_a_case_is_a_pure_function_of_its_index(drawn_cases):
    kept = [index for index in (0, 1, 7, 15, 33, 59, 1234) if ps.draw(index) is not None]
    assert len(kept) >= 4
    ps.draw(kept[-1])   # (an earlier draw does not change a later one)
    for index in kept:
        assert ps.case_bytes(ps.draw(index)) == ps.case_bytes(ps.draw(index)), index
        if index < N_INDICES:
            assert ps.case_bytes(ps.draw(index)) == ps.case_bytes(drawn_cases[index]), index
    assert ps.case_bytes(ps.draw(kept[0])) != ps.case_bytes(ps.draw(kept[1]))


def test_the_two_grids_line_up(drawn_cases):
    """From the oracle alone: the same row count under every request's range, and for an x in series order the same
    timestamps row by row."""
    for drawn in drawn_cases:
        if drawn is None:
            continue
        x, y = drawn.x, drawn.y
        assert len(x.ts) == len(y.ts) <= ps.MAX_ROWS, drawn.index
        for request in drawn.requests:
            t_lo, t_hi = ps.time_bounds(request)
            assert int(x.in_range(t_lo, t_hi).sum()) == int(y.in_range(t_lo, t_hi).sum()), (drawn.index, request.style)
        if not drawn.permuted:
            assert np.array_equal(x.ts, y.ts), drawn.index
        if drawn.kind == "self":
            assert y is x and y.batch is x.batch
        elif drawn.kind == "negated" and not drawn.permuted:
            finite = np.isfinite(x.values)
            assert (y.values[finite] == -x.values[finite]).all(), drawn.index
        # the common cut rows are segment boundaries of both fields (x: in series order only)
        for row in drawn.common_rows:
            if row is not None:
                assert row in y.starts or drawn.kind == "self", drawn.index
                assert drawn.permuted or row in x.starts, drawn.index


def test_at_most_a_third_of_the_indices_is_left_out(drawn_cases):
    left_out = [index for index, drawn in enumerate(drawn_cases) if drawn is None]
    print(f"{len(left_out)} of {N_INDICES} indices left out for more than {ps.MAX_ROWS} rows")
    assert 3 * len(left_out) <= N_INDICES, left_out


def test_few_cells_are_ill_conditioned(census):
    _, cells = census
    for operator, (ill, finite) in cells.items():
        print(f"{operator}: {ill} of {finite} non-empty finite cells are ill-conditioned ({100.0 * ill / finite:.3f} %)")
        assert finite > 1000 and ill <= ILL_CONDITIONED_CAP * finite, operator


def test_the_census_has_no_empty_line(census):
    counts, _ = census
    for name, count in sorted(counts.items()):
        print(f"{name}: {count}")
    wanted = ["x segments: " + name for name in ps.PATHS] + ["t_lo strictly inside an x segment: " + name for name in ps.PATHS]
    wanted += ["binned calls whose keys do not ascend", "binned cells fed by more than one run and more than one segment",
               "edges equal to a value on a Swing line", "rows with a NaN in x only", "rows with a NaN in y only",
               "rows with +inf in y", "rows with -inf in y", "buckets of width 1", "permuted x", "tails", "list cuts",
               "slice sizes", "comoments cells with a non-finite point"]
    wanted += ["kind " + kind for kind in ps.KINDS] + ["grouping " + name for name in ps.GROUPINGS]
    wanted += ["requests of style " + style for style in ps.STYLES]
    empty = [name for name in wanted if counts[name] <= 0]
    assert not empty, empty


def _reference_cells(drawn_cases, limit):
    """(comoments cells, binned cells) as the libraries' records, from the exact references: non-empty finite cells."""
    co, mo = [], []
    for drawn in drawn_cases:
        if drawn is None:
            continue
        for request in drawn.requests[:2]:
            expected = ps.reference_comoments(drawn, request)
            for where in zip(*np.nonzero((expected["count"] > 0) & expected["finite_x"] & expected["finite_y"])):
                co.append((expected["count"][where],) + tuple(expected[name][where] for name in cc.MEMBERS))
            expected = ps.reference_binned(drawn, request)
            for where in zip(*np.nonzero((expected["count"] > 0) & expected["finite"])):
                mo.append((expected["count"][where], expected["mean"][where], expected["m2"][where]))
        if len(co) >= limit and len(mo) >= limit:
            break
    return (np.array(co[:limit], dtype=mdb.COMOMENTS_CELL_DTYPE), np.array(mo[:limit], dtype=mdb.MOMENTS_CELL_DTYPE))


def test_the_python_port_of_the_merge_rules_gives_the_librarys_bytes(drawn_cases):
    co, mo = _reference_cells(drawn_cases, 4000)
    assert len(co) >= 1000 and len(mo) >= 1000
    for cells, merge, ours in ((co, mdb.comoments_merge, ps.merge_comoments), (mo, mdb.moments_merge, ps.merge_moments)):
        half = len(cells) // 2
        a, b = cells[:half].copy(), cells[half:2 * half].copy()
        b[::7] = 0   # (empty sides, either way round)
        a[3::11] = 0
        for into, from_ in ((a, b), (b, a), (a, a)):
            assert ps.merged_arrays(into, from_, ours).tobytes() == merge(into.copy(), from_).tobytes()


def test_the_merge_without_its_cross_term_is_caught():
    """Mutation 1 of the soak, host side: comoments_merge without dx * dy * (na * nb / n) misses the reference of two
    shards by far more than C_TOLERANCE, and differs from mdb.comoments_merge."""
    def mutated(a, b):
        good = ps.merge_comoments(a, b)
        return good if a[0] == 0 or b[0] == 0 else good[:5] + (a[5] + b[5],)
    rng = np.random.default_rng(ps.SEED)
    x, y = rng.normal(100.0, 5.0, 64).astype(np.float32), rng.normal(-3.0, 2.0, 64).astype(np.float32)
    y[32:] += x[32:]   # (the halves differ in both means)
    x[32:] += np.float32(20.0)
    halves = [np.array([(32,) + cc.cell_reference(x[a:a + 32], y[a:a + 32])], dtype=mdb.COMOMENTS_CELL_DTYPE) for a in (0, 32)]
    whole = cc.cell_reference(x, y)
    scale = np.sqrt(whole[2] * whole[3])
    good = mdb.comoments_merge(halves[0].copy(), halves[1])
    assert abs(good["c_xy"][0] - whole[4]) <= cc.C_TOLERANCE * scale
    assert ps.merged_arrays(halves[0], halves[1], ps.merge_comoments).tobytes() == good.tobytes()
    bad = ps.merged_arrays(halves[0], halves[1], mutated)
    assert abs(bad["c_xy"][0] - whole[4]) > 1000 * cc.C_TOLERANCE * scale and bad.tobytes() != good.tobytes()


def test_the_references_agree_with_each_other(drawn_cases):
    """binned_cases.oracle folded over the value cells against comoments_cases.oracle: the count exactly, the y mean and
    m2 within the moments' tolerance; and the counts summed over the cells."""
    checked = 0
    for drawn in drawn_cases:
        if drawn is None:
            continue
        for request in drawn.requests:
            co, bi = ps.reference_comoments(drawn, request), ps.reference_binned(drawn, request)
            assert np.array_equal(bi["count"].sum(axis=2), co["count"]), drawn.index
            cells = mdb.fresh_moments_cells(bi["count"].shape)
            finite = bi["finite"].all(axis=2) & co["finite_y"] & co["finite_x"]   # (the oracle fills finite pairs only)
            cells["count"], cells["mean"], cells["m2"] = bi["count"], bi["mean"], bi["m2"]
            folded = ps.folded_binned(cells)
            assert np.array_equal(folded["count"], co["count"]), drawn.index
            keep = finite & (co["count"] > 0)
            assert (np.abs(folded["mean"] - co["mean_y"])[keep] <= cc.MEAN_TOLERANCE * co["largest_y"][keep]).all(), drawn.index
            assert (np.abs(folded["m2"] - co["m2_y"])[keep] <= cc.M2_TOLERANCE * co["m2_y"][keep]).all(), drawn.index
            checked += int(keep.sum())
    assert checked > 1000


def test_a_zero_mean_has_no_sign_to_negate():
    """A limit of the documented rule, pinned at index 15: y = -x gives mean_y the bytes of
    -mean_x except where the mean is zero. A run of x = 0.0 has mean K + s / n = 0.0 + 0.0, a run of y = -0.0 has
    -0.0 + 0.0: both +0.0, so mean_y is not -(+0.0). Everything else of the negation law holds in the emulation:
    m2_y has m2_x's bytes and c_xy is -m2_x, never positive."""
    drawn = ps.draw(15)
    assert drawn.kind == "negated" and not drawn.permuted
    zeros = 0
    for request in drawn.requests:
        expected, rule = ps.reference_comoments(drawn, request), ps.rule_cells(drawn, request)
        plain = (expected["count"] > 0) & expected["finite_x"] & expected["finite_y"]
        differs = plain & (rule["mean_y"].view(np.uint64) != (-rule["mean_x"]).view(np.uint64))
        assert ((rule["mean_x"][differs] == 0.0) & (rule["mean_y"][differs] == 0.0)).all()
        assert (np.signbit(rule["mean_x"][differs]) == np.signbit(rule["mean_y"][differs])).all()
        zeros += int(differs.sum())
        assert rule["m2_y"][plain].tobytes() == rule["m2_x"][plain].tobytes()
        assert (rule["c_xy"][plain] <= 0.0).all() and (rule["c_xy"][plain] == -rule["m2_x"][plain]).all()
    assert zeros > 0
