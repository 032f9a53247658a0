"""The sequential restatement of lf_map_polylines (tests/map_polylines_ref.py) alone, no GPU: the structure of what it returns,
that the inputs the GPU tests share reach every branch of the contract, the prototype's figures on the track case, and where the
contract gives one polyline per lane and where it does not."""
import numpy as np
import pytest

import map_lanes_ref as L
import map_near_ref as N
import map_polylines_ref as P


def run(ground, colour, shuffle=1, **cfg):
    m, size = P.as_map(ground, colour, shuffle=shuffle)
    return L.cached(("polylines", ground.tobytes(), shuffle, tuple(sorted(cfg.items()))), lambda: P.polylines(m, size, P.config(**cfg), detail=True))


def structure(r):
    """what holds of every result"""
    res, vertex_of, vt, pt, s = r
    val, adj = s["val"], s["adj"]
    part = np.array(s["part"], np.int64)
    # every participating entry is in exactly one vertex, the others in none
    assert res["n_participating"] == len(part) == sum(len(rows) for rows in s["vertex"].values()) == int((vertex_of >= 0).sum())
    assert sorted(t for rows in s["vertex"].values() for t in rows) == list(part)
    assert (vt["n_entries"][vertex_of[part]].sum() if len(part) else 0) == sum(v["n"] ** 2 for v in val.values())
    assert all(vt["first_row"][vertex_of[t]] == val[(int(s["lane_of"][t]),) + s["assigned"][t]]["first_row"] for t in part)
    # every vertex is in exactly one polyline, and the polylines tile the table in ascending smallest first_row
    assert res["n_vertices"] == len(vt) == len(val) == int(pt["n_vertices"].sum()) and res["n_polylines"] == len(pt)
    assert list(pt["first_vertex"]) == list(np.cumsum(pt["n_vertices"]) - pt["n_vertices"])
    assert (np.diff(pt["first_row"]) > 0).all() and len(set(vt["first_row"])) == len(vt)
    assert res["n_edges"] == int((pt["n_vertices"] - 1 + pt["closed"]).sum()) and res["n_closed"] == int(pt["closed"].sum())
    # degree <= 2, and the relation is symmetric
    assert all(len(a) <= 2 and len(set(a)) == len(a) and all(k in adj[u] for u in a) for k, a in adj.items())
    key_of = {v["first_row"]: k for k, v in val.items()}
    for k, p in enumerate(pt):
        v = vt[p["first_vertex"]:p["first_vertex"] + p["n_vertices"]]
        keys = [key_of[f] for f in v["first_row"]]
        assert (v["polyline"] == k).all() and (v["lane"] == p["lane"]).all() and p["first_row"] == v["first_row"].min()
        assert p["n_entries"] == v["n_entries"].sum() and p["hits"] == v["hits"].sum()
        assert all(b in adj[a] for a, b in zip(keys, keys[1:]))                                   # consecutive vertices share an edge
        if p["closed"]:
            assert len(v) >= 3 and keys[0] in adj[keys[-1]] and all(len(adj[q]) == 2 for q in keys)
            assert v["first_row"][0] == p["first_row"]                                            # a cycle starts at its smallest vertex
            assert v["first_row"][1] == min(val[q]["first_row"] for q in adj[keys[0]])            # and goes to the smaller neighbour first
        else:
            assert len(adj[keys[0]]) <= 1 and len(adj[keys[-1]]) <= 1 and all(len(adj[q]) == 2 for q in keys[1:-1])
            assert v["first_row"][0] <= v["first_row"][-1]                                        # a path starts at the smaller end
    assert not (np.signbit(vt["x"]) & (vt["x"] == 0)).any() and not (np.signbit(vt["tx"]) & (vt["tx"] == 0)).any()
    assert (vt["tx"] >= 0).all() and np.allclose(np.hypot(vt["tx"], vt["ty"])[(vt["tx"] != 0) | (vt["ty"] != 0)], 1.0, atol=1e-12)
    return r


def test_the_track_case_gives_the_prototype_figures():
    res, vertex_of, vt, pt, s = structure(P.track_want())
    assert res == {"size": 2036, "n_lanes": 5, "n_participating": 2027, "n_vertices": 505, "n_polylines": 5, "n_closed": 2, "n_edges": 502, "reserved_": 0}
    assert list(pt["n_vertices"]) == [188, 66, 162, 83, 6] and list(pt["closed"]) == [1, 0, 1, 0, 0] and sorted(pt["lane"]) == [0, 1, 2, 3, 4]
    # the closed ones are the two white circles of 2.8 m and 3.3 m
    for k, radius in ((0, None), (2, None)):
        xy = P.polyline_xy(vt, pt, k)
        r = np.hypot(xy[:, 0], xy[:, 1])
        assert r.max() - r.min() < 0.05 and min(abs(r.mean() - 2.8), abs(r.mean() - 3.3)) < 0.02
        step = np.hypot(*np.diff(np.vstack([xy, xy[:1]]), axis=0).T)
        assert step.max() <= 0.3 and 2 * np.pi * r.mean() * 0.97 < step.sum() < 2 * np.pi * r.mean() * 1.03      # once round, in order


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 11])
@pytest.mark.parametrize("cell", [0.05, 0.10, 0.20])
def test_one_polyline_per_lane_on_the_track(seed, cell):
    m, size = L.track_case(seed)
    res, vertex_of, vt, pt, s = structure(P.polylines(m, size, P.config(cell=cell, max_gap=max(0.30, 3 * cell)), detail=True))
    assert res["n_polylines"] == res["n_lanes"] == 5 and sorted(pt["lane"]) == [0, 1, 2, 3, 4] and res["n_closed"] == 2


@pytest.mark.parametrize("angle", [0.0, 45.0, 90.0, 90.6, 115.0])
def test_one_polyline_per_lane_on_straight_lines(angle):
    res, vertex_of, vt, pt, s = structure(run(*P.line_case(angle)))
    assert res["n_polylines"] == res["n_lanes"] >= 1 and sorted(pt["lane"]) == list(range(res["n_lanes"]))


def test_one_polyline_on_a_cell_boundary_and_what_migration_is_for():
    g, c = P.line_case(0.0, at=(0.0, 0.0), jitter=0.01, seed=2)
    res, vertex_of, vt, pt, s = structure(run(g, c))
    assert res["n_polylines"] == 1
    homes = {(int(s["lane_of"][t]),) + s["home"][t] for t in s["part"]}
    assert len(homes) > 1.5 * res["n_vertices"]                              # one vertex per home cell would be a ladder of two rows
    assert {h[2] for h in homes} == {-1, 0} and len(set(vt["cy"])) == 2


def test_one_polyline_on_the_corner_per_lane():
    res, vertex_of, vt, pt, s = structure(run(*P.corner_case()))
    assert res["n_polylines"] == res["n_lanes"] and sorted(pt["lane"]) == list(range(res["n_lanes"]))


# (sigma, y0): the polylines that bands of 4 000 copies with seeds 2, 3 and 4 fall into, at cell 0.10.  y0 = 0 centres the band on a
# cell boundary, 0.05 in a row of cells, 0.025 lies in between.
BANDS = {(0.01, 0.0): [1, 1, 1],
         (0.02, 0.0): [1, 1, 1], (0.02, 0.025): [1, 1, 1], (0.02, 0.05): [1, 1, 1],
         (0.03, 0.0): [5, 2, 2], (0.03, 0.025): [1, 1, 1], (0.03, 0.05): [1, 1, 1],
         (0.04, 0.0): [23, 13, 15], (0.04, 0.025): [8, 5, 3], (0.04, 0.05): [1, 2, 1]}


@pytest.mark.parametrize("sigma,y0", sorted(BANDS))
def test_bands(sigma, y0):
    """Where a band of copies is one polyline and where it is not, over positions in the grid and seeds.  One polyline wherever
    the band lies holds up to a sigma of 0.02 m, a fifth of the cell: nearly all of the band (4 sigma) is narrower than one cell.
    At 0.03 m a band centred on a cell boundary fragments, at 0.04 m every position does for some seed.  Why: the two rows next to
    the boundary hold about equal counts, so the lighter row's entries move into the heavier one -- and the thin tail in the row
    beyond the lighter one moves INTO the lighter row (the heaviest of ITS three cells), which the one-level rule then leaves as a
    row of stray vertices beside the line.  The figures are the restatement's own, recorded so that a change of the contract shows."""
    got = []
    for seed in (2, 3, 4):
        res, vertex_of, vt, pt, s = structure(run(*P.band_case(sigma=sigma, y0=y0, seed=seed)))
        assert res["n_lanes"] == 1 and pt["n_entries"].sum() == 4000
        got.append(res["n_polylines"])
        if res["n_polylines"] == 1:
            assert pt["n_vertices"][0] == 40
    assert got == BANDS[(sigma, y0)]
    assert (max(got) == 1) == (sigma <= 0.02 or (sigma == 0.03 and y0 != 0.0))


def test_a_wide_band_fragments_in_the_best_position():
    assert run(*P.band_case(sigma=0.08, y0=0.05))[0]["n_polylines"] > 1


def test_the_inputs_reach_every_branch():
    track = P.track_want()[4]
    assert {True, False} <= set(track["horizontal"].values())                                     # both lateral axes
    assert {-1, 0, 1} <= set(track["moved"].values())                                             # migration by -1, 0 and +1
    assert {"first", "second-", "second+"} <= {v["branch"] for v in track["val"].values()}        # both half-angle branches, s < 0 in the second
    tie = structure(run(*P.tie_case(), **P.ANY))[4]
    assert sum(1 for t in tie["part"] if tie["tie"][t] and tie["moved"][t] == -1) == 20           # an equal-count tie that moves
    assert sum(1 for t in tie["part"] if tie["tie"][t] and tie["moved"][t] == 0) == 20            # and the same tie seen from the cell that stays
    fan = structure(run(*P.fan_case(), shuffle=None, **P.ANY))
    assert [v["branch"] for v in fan[4]["val"].values()].count("none") == 1                       # h == 0
    assert len(fan[4]["on_neither"]) == 2                                                         # a == 0, from both ends
    fork = structure(run(*P.fork_case()))[4]
    one_sided = [(k, u) for k in fork["val"] for u in (fork["fwd"][k], fork["bwd"][k]) if u is not None and k not in (fork["fwd"][u], fork["bwd"][u])]
    assert one_sided and fork["lanes_res"][0]["n_lanes"] == 1                                     # a one-sided choice that the mutual test drops
    assert run(*P.fork_case())[0]["n_polylines"] == 2


def test_the_small_shapes():
    res, vertex_of, vt, pt, s = structure(run(*P.small_shapes_case(), shuffle=None, **P.ANY))
    assert list(pt["n_vertices"]) == [3, 2, 1] and list(pt["closed"]) == [1, 0, 0] and res["n_edges"] == 4
    assert list(vt["first_row"][:3]) == [0, 1, 2]                                                 # from the smallest vertex to its smaller neighbour
    structure(run(*P.small_shapes_case(), shuffle=3, **P.ANY))
    structure(run(*P.crossing_case()))
    structure(run(*P.pile_case(), shuffle=None))


@pytest.mark.parametrize("n", [63, 1025])
def test_counted_vertices(n):
    res, vertex_of, vt, pt, s = structure(run(*P.counted_case(n), shuffle=None, **P.ANY))
    assert (res["n_vertices"], res["n_polylines"], res["n_edges"]) == (n, 1, n - 1)


def test_the_loaded_table_makes_probes_collide():
    """the GPU test's input for a table at its highest load: 4 000 keys in 8 192 slots, where a model of the probe (linear, from
    slot_hash) meets keys that share their first slot and chains of several steps"""
    g, c = P.loaded_case()
    res, vertex_of, vt, pt, s = run(g, c, shuffle=None, **P.ANY)
    assert res["n_vertices"] == 4000 and P.table_slots(4000) == 8192 and P.table_slots(4096) == 8192 and P.table_slots(4097) == 16384
    assert P.table_slots(0) == P.table_slots(32) == 64 and P.table_slots(33) == 128
    keys = [(int(s["lane_of"][t]),) + s["assigned"][t] for t in s["part"]]
    probes, shared = P.probe_model(keys, 4000)
    assert len(set(keys)) == 4000 and shared > 400 and max(probes) >= 4 and 1.1 < np.mean(probes) < 2.0
    assert P.slot_hash(0, 0, 0) == 0 and P.slot_hash(1, -2, 3) == P.slot_hash(1, 2 ** 32 - 2, 3)  # cells enter as their 32 bits


def test_the_clamp_margin():
    m, size = L.lattice_case("clamped_1e15")
    res, vertex_of, vt, pt, s = structure(P.polylines(m, size, P.config(min_entries=2, **L.WIDE), detail=True))
    assert res["n_lanes"] > 0 and res["n_participating"] == 0 and (vertex_of == -1).all() and len(vt) == 0 and len(pt) == 0
    # the margin itself: the last cell that participates is INT32_MAX - reach - 2
    for reach in (1, 3, 8):
        edge = N.INT32_MAX - reach - 2
        g, c = P.marks([[(edge + 0.5) * 1.0, 0.5], [(edge + 1.5) * 1.0, 0.5]], length=0.5)
        m, size = P.as_map(g, c)
        r = P.polylines(m, size, P.config(cell=1.0, max_gap=2.0, reach=reach, radius=1.5, **P.ANY), detail=True)
        assert r[0]["n_lanes"] == 1 and list(r[1][:2]) == [0, -1] and r[2]["cx"][0] == edge


def test_the_configuration_checks():
    assert P.bad_config(P.config()) is None
    for kw in P.BAD_CONFIGS:
        assert P.bad_config(P.config(**kw)) is not None, kw
    for kw in (dict(cell=2.0 ** -10), dict(cell=16.0), dict(reach=1), dict(reach=8), dict(max_gap=1e-300)):
        assert P.bad_config(P.config(**kw)) is None, kw
    with pytest.raises(TypeError):
        P.config(cells=1)
