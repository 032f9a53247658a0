"""Loop closures for the live map: a pose graph over KEY poses, solved on the device (LineAssociator.graph_solve) and applied to
the map (LineAssociator.correct).

One key per batch is the usual choice: `add_key(step, pose)` with the step that batch was handed to `LineAssociator.step` with
(the entries it wrote carry it as last_seen) and the pose the batch was drawn at.  Consecutive keys are tied by odometry edges,
`add_loop` / `loop_from_localize` add what `LineAssociator.localize` finds in an old part of the map, `solve` spreads the
discrepancy over the trajectory and `apply` moves the map's entries with their keys.
"""
import numpy as np


class PoseGraph(object):
    def __init__(self, odo_w=(100.0, 100.0, 100.0), loop_w=(100.0, 100.0, 100.0)):
        """odo_w / loop_w: the weights (1 / m^2, 1 / m^2, 1 / rad^2) of an odometry edge's and, by default, a loop edge's residuals:
        starting values that no log has tuned, as lf_smooth_config's."""
        self.odo_w = tuple(float(v) for v in odo_w)
        self.loop_w = tuple(float(v) for v in loop_w)
        self.key_step, self.key_pose = [], []
        self.edges, self.z, self.w, self.robust = [], [], [], []
        self.solved = None
        self.result = None

    @staticmethod
    def relative(pa, pb):
        """The measurement of an edge a -> b that the poses pa, pb satisfy: pb in pa's frame, (c ux + s uy, -s ux + c uy,
        th_b - th_a) with (s, c) = sin, cos of th_a and (ux, uy) = b - a; numpy float64, theta not wrapped."""
        pa, pb = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
        s, c = np.sin(pa[2]), np.cos(pa[2])
        ux, uy = pb[0] - pa[0], pb[1] - pa[1]
        return np.array([c * ux + s * uy, (-s) * ux + c * uy, pb[2] - pa[2]])

    def __len__(self):
        return len(self.key_step)

    def add_key(self, step, pose):
        """A node: the key observed at `step` (strictly increasing) from `pose` (x, y, theta), and an odometry edge from the
        previous key with z = relative(previous pose, pose).  Returns the key's index."""
        step = int(step)
        if self.key_step and step <= self.key_step[-1]:
            raise ValueError("add_key: steps are strictly increasing")
        pose = np.array(pose, np.float64).reshape(3)
        if self.key_pose:
            self._edge(len(self.key_pose) - 1, len(self.key_pose), self.relative(self.key_pose[-1], pose), self.odo_w, False)
        self.key_step.append(step)
        self.key_pose.append(pose)
        return len(self.key_step) - 1

    def _edge(self, a, b, z, w, robust):
        self.edges.append((int(a), int(b)))
        self.z.append(np.array(z, np.float64).reshape(3))
        self.w.append(np.array(w, np.float64).reshape(3))
        self.robust.append(1 if robust else 0)

    def add_loop(self, a, b, z, w=None, robust=True):
        """An edge between the keys a and b (a != b): z the pose of b in a's frame."""
        n = len(self.key_step)
        if not (0 <= a < n and 0 <= b < n and a != b):
            raise ValueError("add_loop: a and b are two different keys")
        self._edge(a, b, z, self.loop_w if w is None else w, robust)

    def loop_from_localize(self, a, b, localized_pose_of_b, w=None, robust=True):
        """The loop edge a -> b from a localisation of key b's frame against the part of the map that key a drew: that part stands
        where a's key pose put it, so z = relative(key_pose[a], localized_pose_of_b)."""
        self.add_loop(a, b, self.relative(self.key_pose[a], localized_pose_of_b), w, robust)

    def key_of_step(self, step):
        """The key an entry with last_seen = step belongs to (lf_map_correct's rule), or -1 before the first key."""
        return int(np.searchsorted(np.asarray(self.key_step, np.int64), int(step), side="right")) - 1

    def entries_before(self, assoc, idx, newest_key):
        """idx with -1 in place of every entry whose key is newer than newest_key or that no key observed (seeded entries): the
        matches into the part of the map that is at least that old, for a localisation against it alone."""
        idx = np.array(idx, np.int32).reshape(-1)
        hit = np.flatnonzero(idx >= 0)
        if len(hit):
            seen = assoc.fetch()["last_seen"][idx[hit]]
            key = np.searchsorted(np.asarray(self.key_step, np.int64), seen, side="right") - 1
            idx[hit[(key < 0) | (key > int(newest_key))]] = -1
        return idx

    def key_of_entries(self, assoc, idx):
        """The key of the most frequent last_seen among the map entries idx (an association's matches; -1 are skipped; of equally
        frequent steps the smallest), or -1 without any."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        idx = idx[idx >= 0]
        if not len(idx):
            return -1
        seen = assoc.fetch()["last_seen"][idx]
        steps, counts = np.unique(seen, return_counts=True)
        return self.key_of_step(steps[int(np.argmax(counts))])

    def solve(self, assoc, fixed=None, **config):
        """Solve the graph with LineAssociator.graph_solve (config: graph_config's overrides).  Returns (poses, result, chi2) and
        keeps the poses for `apply`; a solve that is not 'ok' keeps none."""
        if not self.key_pose:
            raise ValueError("solve: no key")
        poses, result, chi2 = assoc.graph_solve(np.stack(self.key_pose), np.array(self.edges, np.int32).reshape(-1, 2),
                                                np.array(self.z, np.float64).reshape(-1, 3), np.array(self.w, np.float64).reshape(-1, 3),
                                                np.array(self.robust, np.uint8), fixed, assoc.graph_config(**config))
        self.result = result
        self.solved = poses if result["status"] == 0 else None
        return poses, result, chi2

    def apply(self, assoc):
        """Move the map with the solved keys (LineAssociator.correct from the key poses to the solved ones) and adopt the solved
        poses as the key poses.  Returns correct's result."""
        if self.solved is None:
            raise ValueError("apply: no accepted solve to apply")
        out = assoc.correct(self.key_step, np.stack(self.key_pose), self.solved)
        self.key_pose = [p.copy() for p in self.solved]
        self.solved = None
        return out
