"""The sequential restatement of lf_map_render / lf_map_bounds (include/lanefront.h "lf_map_render").

A painter's algorithm: the drawn entries are sorted by (last_seen, slot) and painted in that order with plain assignment, the
trajectory last -- on purpose a different mechanism from the kernels' maximum of keys.  Pixel mapping is numpy float64 (a
subtraction, then a multiplication, then floor); lines are the closed form of the midpoint line in Python integers.
"""
import numpy as np

WHITE, YELLOW, RED, BLUE = (255, 255, 255), (0, 255, 255), (0, 0, 255), (255, 0, 0)
LIMIT = float(2 ** 28)


def default_view(**kw):
    """lf_map_default_view as a dict (the reference's map_view.rviz: TopDownOrtho, Scale 30, background 48; 48; 48)."""
    v = dict(rows=512, cols=512, pixels_per_metre=30.0, thickness=1, min_hits=1, min_last_seen=-1, color_mask=0xF, background=(48, 48, 48))
    v.update({k: kw[k] for k in kw if k not in ("x_min", "y_max")})
    v["x_min"] = kw.get("x_min", -v["cols"] / (2 * v["pixels_per_metre"]))
    v["y_max"] = kw.get("y_max", v["rows"] / (2 * v["pixels_per_metre"]))
    return v


def pixel(view, x, y):
    """(u, v) as float64 floors: column and row of the map-frame point (x, y)."""
    x, y = np.float64(x), np.float64(y)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.floor((x - np.float64(view["x_min"])) * np.float64(view["pixels_per_metre"]))
        v = np.floor((np.float64(view["y_max"]) - y) * np.float64(view["pixels_per_metre"]))
    return u, v


def pixel_line(view, g):
    """(u0, v0, u1, v1) as Python ints, or None when the line is skipped."""
    f = pixel(view, g[0], g[1]) + pixel(view, g[2], g[3])
    if not all(np.isfinite(c) and abs(c) < LIMIT for c in f):
        return None
    return tuple(int(c) for c in f)


def line_pixels(u0, v0, u1, v1):
    """The pixels of the line, in order i = 0 .. n."""
    dx, dy = u1 - u0, v1 - v0
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    if abs(dx) >= abs(dy):
        n = abs(dx)
        return [(u0 + i * sx, v0 + sy * ((2 * i * abs(dy) + n) // (2 * n))) for i in range(n + 1)] if n else [(u0, v0)]
    n = abs(dy)
    return [(u0 + sx * ((2 * i * abs(dx) + n) // (2 * n)), v0 + i * sy) for i in range(n + 1)]


def _clipped_steps(u0, v0, u1, v1, rows, cols, t):
    """The range of i whose squares can reach the image (a restriction of i: the pixels themselves do not change)."""
    dx, dy = u1 - u0, v1 - v0
    xmajor = abs(dx) >= abs(dy)
    a0, s, n, size = (u0, (dx > 0) - (dx < 0), abs(dx), cols) if xmajor else (v0, (dy > 0) - (dy < 0), abs(dy), rows)
    lo, hi = -(t // 2), size - 1 + (t - 1) // 2
    if s > 0:
        ia, ib = lo - a0, hi - a0
    elif s < 0:
        ia, ib = a0 - hi, a0 - lo
    else:
        ia, ib = 0, (0 if lo <= a0 <= hi else -1)
    return max(ia, 0), min(ib, n)


def paint_line(img, p, t, bgr, clip=True):
    u0, v0, u1, v1 = p
    rows, cols = img.shape[:2]
    dx, dy = u1 - u0, v1 - v0
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    xmajor = abs(dx) >= abs(dy)
    n, m = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    ia, ib = _clipped_steps(u0, v0, u1, v1, rows, cols, t) if clip else (0, n)
    h0, h1 = (t - 1) // 2, t // 2
    for i in range(ia, ib + 1):
        k = (2 * i * m + n) // (2 * n) if n else 0
        u, v = (u0 + i * sx, v0 + sy * k) if xmajor else (u0 + sx * k, v0 + i * sy)
        r_a, r_b, c_a, c_b = max(v - h0, 0), min(v + h1, rows - 1), max(u - h0, 0), min(u + h1, cols - 1)
        if r_a <= r_b and c_a <= c_b:
            img[r_a:r_b + 1, c_a:c_b + 1] = bgr


def selected(view, color, hits, last_seen):
    c = np.minimum(np.asarray(color).astype(np.int64), 3)
    return (np.asarray(hits) >= view["min_hits"]) & (np.asarray(last_seen) >= view["min_last_seen"]) & (((view["color_mask"] >> c) & 1) == 1)


def render(view, ground, color, hits, last_seen, trajectory=None):
    """(image [rows][cols][3] uint8 BGR, n_drawn, n_skipped) of the entries given in slot order (the arrays of lf_map_fetch, cut to the
    map's size)."""
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    img = np.empty((view["rows"], view["cols"], 3), np.uint8)
    img[:] = np.asarray(view["background"], np.uint8)
    t = view["thickness"]
    sel = selected(view, color, hits, last_seen) if len(ground) else np.zeros(0, bool)
    n_drawn = n_skipped = 0
    todo = []
    for slot in np.nonzero(sel)[0]:
        p = pixel_line(view, ground[slot])
        if p is None:
            n_skipped += 1
            continue
        n_drawn += 1
        todo.append((int(last_seen[slot]), int(slot), p))
    for _, slot, p in sorted(todo):
        c = int(color[slot])
        paint_line(img, p, t, WHITE if c == 0 else YELLOW if c == 1 else RED)
    if trajectory is not None:
        tr = np.asarray(trajectory, np.float64).reshape(-1, 2)
        for j in range(len(tr) - 1):
            p = pixel_line(view, (tr[j, 0], tr[j, 1], tr[j + 1, 0], tr[j + 1, 1]))
            if p is None:
                n_skipped += 1
                continue
            n_drawn += 1
            paint_line(img, p, t, BLUE)
    return img, n_drawn, n_skipped


def bounds(ground, color, hits, last_seen, view=None):
    """((xmin, ymin, xmax, ymax) or None, n_entries): over the endpoints with both coordinates finite of the selected entries."""
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    sel = selected(view, color, hits, last_seen) if view is not None else np.ones(len(ground), bool)
    pts = ground[sel].reshape(-1, 2, 2)
    ok = np.isfinite(pts).all(axis=2)
    n = int(ok.any(axis=1).sum())
    if not n:
        return None, 0
    good = pts[ok]
    return (float(good[:, 0].min()), float(good[:, 1].min()), float(good[:, 0].max()), float(good[:, 1].max())), n


def fnv1a(data):
    """64-bit FNV-1a of a bytes-like object (what tests/c_abi/map_render_client.c prints of its image)."""
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
