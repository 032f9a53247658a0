"""Inputs for the frame-motion tests (no detector): batches of frames as the arrays lf_motion_estimate reads.  Plain numpy: input
makers, not a contract.

  circuit(frames)        frames of tests/map_loop_scene.Scene, the closed circuit with marks along one line and across the other:
                         lines in two directions, unique codes, noiseless ground points in the robot frames
  straight_road(...)     marks along two parallel lines only: the search is degenerate by design
  random_batch(...)      frames of given lengths with random ground points and codes; alphabet > 0 draws the codes from that many
                         distinct ones, so that equal codes and equal distances abound
"""
import types

import numpy as np

import map_loop_scene as S


def batch(frame_offset, ground, color, keep, code, **more):
    """the arrays as an object FrameMotion.estimate takes for a host `Segments` block"""
    code = np.ascontiguousarray(code, np.uint8).reshape(-1, 32)
    return types.SimpleNamespace(n=len(code), frame_offset=np.ascontiguousarray(frame_offset, np.int32),
                                 ground=np.ascontiguousarray(ground, np.float64).reshape(-1, 4),
                                 color=None if color is None else np.ascontiguousarray(color, np.uint8),
                                 keep=None if keep is None else np.ascontiguousarray(keep, np.uint8), code=code, **more)


def from_frames(world, color, code, seen, poses):
    """one frame per pose: the marks seen[k] of the world, in the robot frame of poses[k]"""
    fo = np.concatenate([[0], np.cumsum([len(s) for s in seen])])
    marks = np.concatenate(seen) if len(seen) else np.zeros(0, np.int64)
    ground = np.concatenate([S.to_robot(world[s], p) for s, p in zip(seen, poses)]) if len(seen) else np.zeros((0, 4))
    return batch(fo, ground, color[marks], None, code[marks], marks=marks, true=np.asarray(poses, np.float64))


def circuit(frames, seed=1):
    sc = S.Scene(seed)
    return from_frames(sc.world, sc.color, sc.code, [sc.seen[k] for k in frames], sc.true[list(frames)])


def straight_road(n_frames=4, step=0.2, view=0.6, seed=2):
    rng = np.random.default_rng(seed)
    x = np.arange(-10, 40) * 0.08
    world = np.concatenate([np.stack([x - 0.03, np.full_like(x, s), x + 0.03, np.full_like(x, s)], 1) for s in (-0.25, 0.25)])
    color = np.concatenate([np.ones(len(x), np.uint8), np.zeros(len(x), np.uint8)])
    code = rng.integers(0, 256, (len(world), 32), dtype=np.uint8)
    poses = np.stack([step * np.arange(n_frames), np.zeros(n_frames), np.zeros(n_frames)], 1)
    mid = 0.5 * (world[:, :2] + world[:, 2:])
    seen = [np.flatnonzero(np.hypot(*(mid - p[:2]).T) < view) for p in poses]
    return from_frames(world, color, code, seen, poses)


def world_batch(sizes, seed, colors=3, shuffle=True):
    """frame k sees the first sizes[k] of max(sizes) random marks (in an order of its own) from a pose of its own: unique codes and
    consistent geometry, so every mark of the shorter frame of a pair has its true match in the other"""
    rng = np.random.default_rng(seed)
    m = int(max(sizes)) if len(sizes) else 0
    mid, ang, half = rng.uniform(-1.0, 1.0, (m, 2)), rng.uniform(0, np.pi, m), rng.uniform(0.02, 0.1, m)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    world = np.concatenate([mid - d, mid + d], 1)
    code = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    color = rng.integers(0, colors, m).astype(np.uint8)
    poses = np.stack([rng.uniform(-0.2, 0.2, len(sizes)), rng.uniform(-0.2, 0.2, len(sizes)), rng.uniform(-0.3, 0.3, len(sizes))], 1)
    seen = [rng.permutation(int(s)) if shuffle else np.arange(int(s)) for s in sizes]
    return from_frames(world, color, code, seen, poses)


def random_batch(sizes, seed, alphabet=0, colors=3, keep_fraction=1.0):
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    fo = np.concatenate([[0], np.cumsum(sizes)])
    ground = rng.uniform(-1.0, 1.0, (n, 4))
    code = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if alphabet:
        code = rng.integers(0, 256, (alphabet, 32), dtype=np.uint8)[rng.integers(0, alphabet, n)]
    color = rng.integers(0, colors, n).astype(np.uint8)
    keep = (rng.random(n) < keep_fraction).astype(np.uint8)
    return batch(fo, ground, color, keep, code)
