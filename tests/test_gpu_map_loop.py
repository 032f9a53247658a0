"""A loop closed end to end on a synthetic circuit (tests/map_loop_scene.py, no detector): one lap and a bit in batches of two frames,
one key per batch, odometry with a constant heading bias; the last batch is localised against the first lap's entries, the loop
edge goes into a PoseGraph, the graph is solved and the map moved.  Afterwards the map's endpoints lie closer to the true lines and
the last key closer to its true pose.  The first test states the same on the CPU, with the restatement and the numpy correction
alone, so that the scene is known to satisfy both inequalities before a GPU sees it.

Measured on the GPU: the mean distance of the endpoints to the true lines falls from 0.2089 m to 0.0340 m, the last key's distance to
its true position from 0.5583 m to 0.0016 m (the CPU statement: 0.2151 -> 0.0341 m and 0.5583 -> 0.0016 m)."""
import math

import numpy as np
import pytest

import map_graph_ref as G
import map_loop_scene as W
from lane_slam_amd.pose_graph import PoseGraph

OLD = 5                              # a loop closes against entries at least this many keys old
LAST = W.N_BATCHES - 1


def compose(pa, rel):
    c, s = math.cos(pa[2]), math.sin(pa[2])
    return np.array([pa[0] + c * rel[0] - s * rel[1], pa[1] + s * rel[0] + c * rel[1], pa[2] + rel[2]])


def graph_of(scene):
    pg = PoseGraph()
    for b in range(W.N_BATCHES):
        pg.add_key(b, scene.key_pose(b))
    return pg


def position_error(scene, pose):
    return float(np.hypot(*(np.asarray(pose)[:2] - scene.key_pose(LAST, odo=False)[:2])))


def test_the_scene_satisfies_both_inequalities_on_the_cpu():
    scene = W.Scene()
    model = scene.model_map(LAST)                                     # batches 0 .. 24 are in the map, the last one is held back
    marks = np.array(sorted(model))
    ground, seen = np.array([model[k][0] for k in marks]), np.array([model[k][1] for k in marks])
    # the last batch's first frame against the entries at least OLD keys old: the key most of them belong to
    first = scene.seen[LAST * W.FRAMES_PER_BATCH]
    old = [model[k][1] for k in first if model[k][1] <= LAST - OLD]
    assert len(old) >= 6
    a = int(np.bincount(old).argmax())
    assert a in (1, 2)
    # what a localisation against that part gives: the part stands where key a's odometry put it
    localized = compose(scene.key_pose(a), PoseGraph.relative(scene.key_pose(a, odo=False), scene.key_pose(LAST, odo=False)))
    pg = graph_of(scene)
    pg.loop_from_localize(a, LAST, localized)
    x, res, chi = G.solve(G.config(), np.stack(pg.key_pose), pg.edges, pg.z, pg.w, robust=pg.robust)
    assert res["status"] == G.OK and res["cost"] < 0.05 * res["cost0"]
    after, moved = G.correct(ground, seen, len(ground), pg.key_step, np.stack(pg.key_pose), x)
    d0, d1 = scene.mean_distance(marks, ground), scene.mean_distance(marks, after)
    e0, e1 = position_error(scene, pg.key_pose[LAST]), position_error(scene, x[LAST])
    print("cpu: endpoints %.4f -> %.4f m, last key %.4f -> %.4f m, moved %d" % (d0, d1, e0, e1, moved["n_moved"]))
    assert d1 < d0 and e1 < e0
    assert d1 < 0.5 * d0 and e1 < 0.5 * e0                          # and by a wide margin: the GPU run has room


@pytest.mark.gpu
def test_a_loop_is_closed_end_to_end():
    import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)
    from lane_slam_amd import LineAssociator
    from test_gpu_map_align import Segs
    scene = W.Scene()
    a = LineAssociator(capacity=1024, policy="merge", merge_distance=0, kept_only=False, color_gating=True)
    try:
        pg = PoseGraph()
        for b in range(LAST):
            marks, fo, ground, poses = scene.batch(b)
            a.step(Segs(scene.code[marks], scene.color[marks], ground, fo), poses, b)
            pg.add_key(b, poses[0])
        marks, fo, ground, poses = scene.batch(LAST)
        b = pg.add_key(LAST, poses[0])
        seg = Segs(scene.code[marks], scene.color[marks], ground, fo)
        idx, dist = a.associate(seg.code, seg.color)
        assert (dist == 0).all() and (idx >= 0).all()
        idx_old = pg.entries_before(a, idx, LAST - OLD)
        assert 6 <= (idx_old >= 0).sum() < len(idx)
        located, loc = a.localize(seg, idx_old, dist, fallback=poses)
        assert loc["status"][0] == 0 and loc["n_inliers"][0] >= a.localize_config().min_inliers
        key = pg.key_of_entries(a, idx_old[fo[0]:fo[1]])
        assert key in (1, 2)
        pg.loop_from_localize(key, b, located[0])

        size = a.state()["size"]
        before = a.fetch(0, size)
        by_code = {scene.code[k].tobytes(): k for k in range(len(scene.code))}
        which = np.array([by_code[c.tobytes()] for c in before["code"]])
        x, res, chi = pg.solve(a)
        assert res["status"] == 0 and res["cost"] < 0.05 * res["cost0"]
        odometry_pose = pg.key_pose[LAST].copy()
        moved = pg.apply(a)
        after = a.fetch(0, size)
        d0, d1 = scene.mean_distance(which, before["ground"]), scene.mean_distance(which, after["ground"])
        e0, e1 = position_error(scene, odometry_pose), position_error(scene, pg.key_pose[LAST])
        print("gpu: endpoints %.4f -> %.4f m, last key %.4f -> %.4f m, moved %d" % (d0, d1, e0, e1, moved["n_moved"]))
        assert d1 < d0 and e1 < e0
        assert moved["n_moved"] + moved["n_left"] == size and moved["n_left"] > 0          # key 0 is fixed: its entries stay
        assert all(after[k].tobytes() == before[k].tobytes() for k in ("code", "color", "hits", "last_seen"))
        assert (np.stack(pg.key_pose) == x).all() and pg.solved is None
    finally:
        a.close()
