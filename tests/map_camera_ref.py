"""The sequential restatement of lf_map_camera_view / lf_map_render_camera (include/lanefront.h "lf_map_render_camera").

Every entry of every frame is projected in plain Python floats (IEEE f64, one rounding per operation, nothing fused) in the order
the header states, then the drawn ones are painted in ascending (last_seen, slot) with plain assignment onto a copy of the source:
a painter's algorithm, on purpose a different mechanism from the kernels' maximum of keys.  The line and the brush are
map_render_ref's.  cos and sin of a pose come from the oracle's own map-frame transform, the routine the device path uses.
"""
import math

import numpy as np

import map_render_ref as R

LIMIT = float(2 ** 28)
DRAWN, CLIP_A, CLIP_B, BEHIND, SKIPPED, FILTERED = "drawn", "clip_a", "clip_b", "behind", "skipped", "filtered"
PALETTE3 = ((255, 255, 255), (0, 255, 255), (0, 0, 255))

_omap = None


def cos_sin(theta):
    """(cs, sn) as the library computes them: the map-frame transform of the unit vectors at pose (0, 0, theta)."""
    global _omap
    if _omap is None:
        from oracle.oracle import OracleMap
        _omap = OracleMap(capacity=64)
    out = _omap.to_map_frame(np.array([[1.0, 0.0, 0.0, 1.0]]), np.array([0, 1], np.int32), np.array([[0.0, 0.0, float(theta)]]))[0]
    cs, sn = float(out[0]), float(out[1])
    assert float(out[3]) == cs and float(out[2]) == -sn
    return cs, sn


def default_hinv(H, cam_w=640, cam_h=480):
    """lf_map_camera_view's hinv: the adjugate over the determinant, scaled so that q_z = 1 at the bottom-centre ground point."""
    a, b, c, d, e, f, g, h, i = (float(x) for x in H)
    adj = [e * i - f * h, c * h - b * i, b * f - c * e,
           f * g - d * i, a * i - c * g, c * d - a * f,
           d * h - e * g, b * g - a * h, a * e - b * d]
    det = (a * adj[0] + b * adj[3]) + c * adj[6]
    inv = [x / det for x in adj]
    gx, gy = bottom_centre_ground(H, cam_w, cam_h)
    s = (inv[6] * gx + inv[7] * gy) + inv[8]
    return [x / s for x in inv]


def bottom_centre_ground(H, cam_w=640, cam_h=480):
    H = [float(x) for x in H]
    pu, pv = float(cam_w // 2), float(cam_h - 1)
    gr = [(H[3 * k] * pu + H[3 * k + 1] * pv) + H[3 * k + 2] for k in range(3)]
    return gr[0] / gr[2], gr[1] / gr[2]


def default_view(H, rows, cols, top_cutoff=0, cam_w=640, cam_h=480, **kw):
    """lf_map_camera_view as a dict."""
    v = dict(rows=rows, cols=cols, top_cutoff=top_cutoff, cam_w=cam_w, cam_h=cam_h, hinv=default_hinv(H, cam_w, cam_h), w_near=0.25,
             thickness=5, min_hits=1, min_last_seen=-1, color_mask=0xF, palette=PALETTE3, background=(48, 48, 48))
    v.update(kw)
    return v


def homogeneous(view, pose, X, Y, cs_sn=None):
    """(q_x, q_y, q_z) of the map-frame point (X, Y) seen from pose = (x, y, theta)."""
    x, y = float(pose[0]), float(pose[1])
    cs, sn = cs_sn if cs_sn is not None else cos_sin(pose[2])
    h = [float(c) for c in view["hinv"]]
    dx, dy = float(X) - x, float(Y) - y
    px = cs * dx + sn * dy
    py = cs * dy - sn * dx
    return [(h[3 * k] * px + h[3 * k + 1] * py) + h[3 * k + 2] for k in range(3)]


def ground2pixel(view, X, Y):
    """The float pixel (q_x / q_z, q_y / q_z) of a robot-frame ground point: the rectified branch of GroundProjection.ground2pixel."""
    q = homogeneous(view, (0.0, 0.0, 0.0), X, Y, (1.0, 0.0))
    return q[0] / q[2], q[1] / q[2]


def project(view, pose, g, cs_sn=None):
    """(category, (u0, v0, u1, v1) as ints or None, the two clipped homogeneous points) of the entry with endpoints g."""
    cs_sn = cs_sn if cs_sn is not None else cos_sin(pose[2])
    a = homogeneous(view, pose, g[0], g[1], cs_sn)
    b = homogeneous(view, pose, g[2], g[3], cs_sn)
    w = float(view["w_near"])
    below_a, below_b = a[2] < w, b[2] < w
    if below_a and below_b:
        return BEHIND, None, (a, b)
    cat = DRAWN
    if below_a:
        t = (w - a[2]) / (b[2] - a[2])
        a = [a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), w]
        cat = CLIP_A
    elif below_b:
        t = (w - b[2]) / (a[2] - b[2])
        b = [b[0] + t * (a[0] - b[0]), b[1] + t * (a[1] - b[1]), w]
        cat = CLIP_B
    sx = float(view["cols"]) / float(view["cam_w"])
    sy = float(view["rows"] + view["top_cutoff"]) / float(view["cam_h"])
    f = []
    for q in (a, b):
        for val in ((q[0] / q[2]) * sx, (q[1] / q[2]) * sy):
            if not math.isfinite(val):
                return SKIPPED, None, (a, b)
            fl = float(math.floor(val))
            if not abs(fl) < LIMIT:
                return SKIPPED, None, (a, b)
            f.append(int(fl))
    return cat, (f[0], f[1] - view["top_cutoff"], f[2], f[3] - view["top_cutoff"]), (a, b)


def select_view(view):
    return dict(min_hits=view["min_hits"], min_last_seen=view["min_last_seen"], color_mask=view["color_mask"])


def render(view, ground, color, hits, last_seen, poses=None, src=None, n_frames=None):
    """(images [n][rows][cols][3] uint8, counts [n][3] = drawn, skipped, behind, categories [n][entries]) of the entries given in slot
    order (the arrays of lf_map_fetch, cut to the map's size)."""
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    if poses is None:
        n = n_frames if n_frames is not None else (len(src) if src is not None else 1)
        poses = np.zeros((n, 3))
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    n = len(poses)
    rows, cols = view["rows"], view["cols"]
    if src is None:
        out = np.empty((n, rows, cols, 3), np.uint8)
        out[:] = np.asarray(view["background"], np.uint8)
    else:
        out = np.array(src, np.uint8, copy=True)
        assert out.shape == (n, rows, cols, 3)
    sel = R.selected(select_view(view), color, hits, last_seen) if len(ground) else np.zeros(0, bool)
    pal = [tuple(int(c) for c in p) for p in view["palette"]]
    counts = np.zeros((n, 3), np.int32)
    cats = []
    for f in range(n):
        cs_sn = cos_sin(poses[f, 2])
        todo, fc = [], []
        for slot in range(len(ground)):
            if not sel[slot]:
                fc.append(FILTERED)
                continue
            cat, p, _ = project(view, poses[f], [float(c) for c in ground[slot]], cs_sn)
            fc.append(cat)
            if cat == BEHIND:
                counts[f, 2] += 1
            elif cat == SKIPPED:
                counts[f, 1] += 1
            else:
                counts[f, 0] += 1
                todo.append((int(last_seen[slot]), slot, p))
        for _, slot, p in sorted(todo):
            R.paint_line(out[f], p, view["thickness"], pal[min(int(color[slot]), len(pal) - 1)])
        cats.append(fc)
    return out, counts, cats
