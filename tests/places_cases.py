"""Inputs for the key-frame store's tests (no detector): batches as tests/frame_motion_cases.py makes them, designed for the places
where the score, the selection and the motion against a stored key can go wrong.  Plain numpy: input makers, not a contract.

  SIZES              segment counts on either side of a wave's turn of 64 and of k_frame_motion's tile of 256
  selection()        one query frame and nine keys whose scores are known by design: equal scores at the top_k boundary, a
                     neighbour that key_gap suppresses, an empty key, the best key of all outside the limit
  loop_scene()       tests/map_loop_scene.Scene's 52 frames with 24 random bits flipped in every observation's code
"""
import numpy as np

import frame_motion_cases as C
import map_loop_scene as S

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 300]
FLIPS = 24


def selection(seed=31):
    """(keys batch, query batch, the scores by design).  Marks have unique random codes (about 128 bits apart), the query frame sees
    marks 0 .. 9, key k the first SEEN[k] marks: with max_distance 64 the score is min(10, SEEN[k]); the last key sees ten others."""
    rng = np.random.default_rng(seed)
    m = 20
    mid, ang = rng.uniform(-1.0, 1.0, (m, 2)), rng.uniform(0, np.pi, m)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * 0.05
    world = np.concatenate([mid - d, mid + d], 1)
    code = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    color = (np.arange(m) % 3).astype(np.uint8)
    seen_counts = [6, 8, 10, 8, 0, 6, 6, 10]
    seen = [rng.permutation(c) for c in seen_counts] + [np.arange(10, 20)]
    poses = np.stack([rng.uniform(-0.2, 0.2, 10), rng.uniform(-0.2, 0.2, 10), rng.uniform(-0.3, 0.3, 10)], 1)
    keys = C.from_frames(world, color, code, seen, poses[:9])
    query = C.from_frames(world, color, code, [rng.permutation(10)], poses[9:])
    return keys, query, np.array(seen_counts + [0], np.int32)


def flipped(code, rng, bits=FLIPS):
    """every row with `bits` distinct random bits flipped"""
    out = np.array(code, np.uint8).reshape(-1, 32).copy()
    for row in out:
        for k in rng.choice(256, bits, replace=False):
            row[k // 8] ^= np.uint8(1 << (k % 8))
    return out


def loop_scene(seed=1):
    """the scene and all its frames as one batch; every observation's code differs from its mark's in 24 bits"""
    sc = S.Scene(seed)
    b = C.from_frames(sc.world, sc.color, sc.code, sc.seen, sc.true)
    b.code = flipped(b.code, np.random.default_rng(seed + 100))
    return sc, b


def odd_ground(b, rng, fraction=0.1):
    """the batch with some ground values non-finite and some segments of zero length (in place); returns the batch"""
    n = b.n
    for rows, value in ((rng.choice(n, max(int(n * fraction / 2), 1), replace=False), None), (rng.choice(n, max(int(n * fraction / 2), 1), replace=False), 0)):
        for r in rows:
            if value is None:
                b.ground[r, rng.integers(0, 4)] = rng.choice([np.nan, np.inf, -np.inf])
            else:
                b.ground[r, 2:] = b.ground[r, :2]
    return b
