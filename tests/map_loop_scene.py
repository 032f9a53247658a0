"""A synthetic closed circuit for the loop-closure tests (no detector): marks with unique codes round a circle, a robot that drives
one lap and a bit in batches of two frames, and odometry with a constant heading bias per frame.  Plain numpy: an input maker, not
a contract.  `model_map` states what a MERGE map holds after the batches were stepped in with their odometry poses (the newest
observation of a mark and its step), so that the scene can be checked on the CPU with tests/map_graph_ref.py alone."""
import math

import numpy as np

R, MARK_STEP, MARK_LEN, SIDE = 3.0, 0.08, 0.06, 0.25
FRAMES_PER_LAP, FRAMES_PER_BATCH, N_BATCHES = 48, 2, 26        # 24 batches are a lap; the last two see what batches 0 and 1 saw
VIEW, BIAS = 0.5, 0.004                                        # metres a mark's midpoint may be away; radians of heading bias per frame


def to_map(ground, pose):
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    out = np.empty_like(ground)
    for e in (0, 2):
        out[:, e], out[:, e + 1] = x + (c * ground[:, e] - s * ground[:, e + 1]), y + (s * ground[:, e] + c * ground[:, e + 1])
    return out


def to_robot(ground, pose):
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    out = np.empty_like(ground)
    for e in (0, 2):
        dx, dy = ground[:, e] - x, ground[:, e + 1] - y
        out[:, e], out[:, e + 1] = c * dx + s * dy, -s * dx + c * dy
    return out


class Scene(object):
    def __init__(self, seed=1):
        rng = np.random.default_rng(seed)
        n = int(2 * math.pi * R / MARK_STEP)
        a = 2 * math.pi * np.arange(n) / n
        rad = np.stack([np.cos(a), np.sin(a)], 1)
        tan = np.stack([-np.sin(a), np.cos(a)], 1)
        inner, outer = (R - SIDE) * rad, (R + SIDE) * rad
        # yellow marks along the inner line, white marks across the outer one: two directions for the localisation
        self.world = np.concatenate([np.concatenate([inner - 0.5 * MARK_LEN * tan, inner + 0.5 * MARK_LEN * tan], 1),
                                     np.concatenate([outer - 0.5 * MARK_LEN * rad, outer + 0.5 * MARK_LEN * rad], 1)])
        self.color = np.concatenate([np.ones(n, np.uint8), np.zeros(n, np.uint8)])
        self.code = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
        n_frames = N_BATCHES * FRAMES_PER_BATCH
        f = 2 * math.pi * np.arange(n_frames) / FRAMES_PER_LAP
        self.true = np.stack([R * np.cos(f), R * np.sin(f), f + math.pi / 2], 1)
        # dead reckoning: the true increments, each turned a little further
        odo = [self.true[0].copy()]
        for k in range(1, n_frames):
            c, s = math.cos(self.true[k - 1, 2]), math.sin(self.true[k - 1, 2])
            dx, dy = self.true[k, :2] - self.true[k - 1, :2]
            zx, zy, zt = c * dx + s * dy, -s * dx + c * dy, self.true[k, 2] - self.true[k - 1, 2] + BIAS
            c, s = math.cos(odo[-1][2]), math.sin(odo[-1][2])
            odo.append(np.array([odo[-1][0] + c * zx - s * zy, odo[-1][1] + s * zx + c * zy, odo[-1][2] + zt]))
        self.odo = np.array(odo)
        mid = 0.5 * (self.world[:, :2] + self.world[:, 2:])
        self.seen = [np.flatnonzero(np.hypot(*(mid - self.true[k, :2]).T) < VIEW) for k in range(n_frames)]

    def batch(self, b):
        """(marks seen per frame concatenated, frame_offset, ground in the robot frames, the frames' odometry poses)"""
        frames = range(b * FRAMES_PER_BATCH, (b + 1) * FRAMES_PER_BATCH)
        marks = np.concatenate([self.seen[k] for k in frames])
        fo = np.concatenate([[0], np.cumsum([len(self.seen[k]) for k in frames])]).astype(np.int32)
        ground = np.concatenate([to_robot(self.world[self.seen[k]], self.true[k]) for k in frames])
        return marks, fo, ground, self.odo[list(frames)]

    def key_pose(self, b, odo=True):
        return (self.odo if odo else self.true)[b * FRAMES_PER_BATCH]

    def model_map(self, n_batches):
        """{mark: (ground in the map frame, step)} after batches 0 .. n_batches - 1: the newest observation wins (MERGE, distance 0)"""
        m = {}
        for b in range(n_batches):
            marks, fo, ground, poses = self.batch(b)
            for f in range(FRAMES_PER_BATCH):
                g = to_map(ground[fo[f]:fo[f + 1]], poses[f])
                for j, mark in enumerate(marks[fo[f]:fo[f + 1]]):
                    m[int(mark)] = (g[j], b)
        return m

    def mean_distance(self, marks, ground):
        """the mean distance of the entries' endpoints to the true lines of their marks"""
        w = self.world[marks]
        d = w[:, 2:] - w[:, :2]
        nrm = np.stack([-d[:, 1], d[:, 0]], 1) / np.hypot(d[:, 0], d[:, 1])[:, None]
        dist = [np.abs(((ground[:, e:e + 2] - w[:, :2]) * nrm).sum(1)) for e in (0, 2)]
        return float(np.mean(dist))
