"""Regenerate tests/golden/lane_filter.npz: the histogram lane filter of the reference itself
(src/lane_filter/include/lane_filter/lane_filter.py, LaneFilterHistogram) driven the way lane_filter_node.processSegments
drives it (src/lane_filter/src/lane_filter_node.py:49-87): predict(dt, v, w) -> update(segments) -> getEstimate / getMax.

Needs a checkout of the reference (argument 1, or $LANE_SLAM_REFERENCE), numpy and scipy.  The reference module is imported
as it is: duckietown_msgs.msg is stubbed by name, duckietown_utils/parameters.py is loaded from the checkout on its own (the
package __init__ pulls in ROS).  The fixture stores numbers only.

    python tests/golden/make_golden_lane_filter.py /path/to/lane-slam
"""
import importlib.util
import math
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lane_filter_ref import PARAM_NAMES, radius  # noqa: E402

DEFAULT = dict(mean_d_0=0, mean_phi_0=0, sigma_d_0=0.1, sigma_phi_0=0.1, delta_d=0.02, delta_phi=0.1, d_max=0.3, d_min=-0.15,
               phi_min=-1.5, phi_max=1.5, cov_v=0.5, linewidth_white=0.05, linewidth_yellow=0.025, lanewidth=0.23, min_max=0.1,
               sigma_d_mask=1.0, sigma_phi_mask=2.0)      # src/duckietown/config/baseline/lane_filter/lane_filter_node/default.yaml
ODD = dict(mean_d_0=0.02, mean_phi_0=0.1, sigma_d_0=0.05, sigma_phi_0=0.2, delta_d=0.03, delta_phi=0.07, d_max=0.25, d_min=-0.2,
           phi_min=-1.0, phi_max=1.2, cov_v=0.5, linewidth_white=0.05, linewidth_yellow=0.025, lanewidth=0.23, min_max=0.05,
           sigma_d_mask=1.5, sigma_phi_mask=0.7)


def load_reference(ref):
    msg = types.ModuleType("duckietown_msgs.msg")

    class Segment(object):
        WHITE, YELLOW, RED = 0, 1, 2
    msg.Segment = Segment
    pkg = types.ModuleType("duckietown_msgs")
    pkg.msg = msg
    sys.modules["duckietown_msgs"], sys.modules["duckietown_msgs.msg"] = pkg, msg
    du = types.ModuleType("duckietown_utils")
    du.__path__ = []
    sys.modules["duckietown_utils"] = du
    spec = importlib.util.spec_from_file_location("duckietown_utils.parameters",
                                                  os.path.join(ref, "src/duckietown/include/duckietown_utils/parameters.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m
    spec.loader.exec_module(m)
    d = os.path.join(ref, "src/lane_filter/include/lane_filter")
    spec = importlib.util.spec_from_file_location("lane_filter", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    lf = importlib.util.module_from_spec(spec)
    sys.modules["lane_filter"] = lf
    spec.loader.exec_module(lf)
    return lf


class _Point(object):
    __slots__ = ("x", "y", "z")


class _Seg(object):
    WHITE, YELLOW, RED = 0, 1, 2

    def __init__(self, color, g):
        self.color = int(color)
        self.points = [_Point(), _Point()]
        self.points[0].x, self.points[0].y, self.points[1].x, self.points[1].y = (float(v) for v in g)


def render(rng, d, phi, lanewidth=0.23, lw_white=0.05, lw_yellow=0.025, n=16, noise=0.004):
    """Ground segments (robot frame, x forward, y left) of the four lane-marking edges seen from lateral offset d and heading
    phi, endpoints ordered the way generateVote reads each edge, plus Gaussian noise."""
    edges = ((0, -lanewidth / 2, False), (0, -(lanewidth / 2 + lw_white), True),
             (1, lanewidth / 2 + lw_yellow, False), (1, lanewidth / 2, True))
    col, g = [], []
    for _ in range(n):
        c, y_l, rev = edges[int(rng.integers(0, 4))]
        s1 = float(rng.uniform(0.1, 0.5))
        s2 = s1 + float(rng.uniform(0.03, 0.12))
        pts = []
        for s in ((s2, s1) if rev else (s1, s2)):
            dx, dy = s, y_l - d
            pts += [math.cos(phi) * dx + math.sin(phi) * dy, -math.sin(phi) * dx + math.cos(phi) * dy]
        col.append(c)
        g.append(np.array(pts) + rng.normal(0, noise, 4))
    return np.array(col, np.uint8), np.array(g, np.float64).reshape(-1, 4)


def run(lf, cfg, steps, init=None):
    F = lf.LaneFilterHistogram(cfg)
    if init is not None:
        F.belief = np.array(init, np.float64)
    out = dict(cfg=np.array([float(cfg[k]) for k in PARAM_NAMES]), init=np.array(F.belief, np.float64))
    from scipy.ndimage import _filters
    out["sin"] = np.sin(F.phi)
    out["wd"] = _filters._gaussian_kernel1d(cfg["sigma_d_mask"], 0, radius(cfg["sigma_d_mask"]))[::-1][radius(cfg["sigma_d_mask"]):].copy()
    out["wphi"] = _filters._gaussian_kernel1d(cfg["sigma_phi_mask"], 0, radius(cfg["sigma_phi_mask"]))[::-1][radius(cfg["sigma_phi_mask"]):].copy()
    dtvw, offs, cols, grounds, pred, post, ml, has_ml, est, in_lane = [], [0], [], [], [], [], [], [], [], []
    for (dt, v, w), (c, g) in steps:
        F.predict(dt=dt, v=v, w=w)
        pred.append(np.array(F.belief, np.float64))
        m = F.update([_Seg(ci, gi) for ci, gi in zip(c, g)])
        post.append(np.array(F.belief, np.float64))
        has_ml.append(m is not None)
        ml.append(np.zeros(F.belief.shape) if m is None else np.array(m, np.float64))
        dm, pm = F.getEstimate()
        mx = F.getMax()
        est.append([dm, pm, mx])
        in_lane.append(mx > F.min_max)
        dtvw.append([dt, v, w])
        offs.append(offs[-1] + len(c))
        cols.append(np.asarray(c, np.uint8))
        grounds.append(np.asarray(g, np.float64).reshape(-1, 4))
    out.update(dtvw=np.array(dtvw, np.float64), seg_offset=np.array(offs, np.int32),
               color=np.concatenate(cols) if cols else np.zeros(0, np.uint8),
               ground=np.concatenate(grounds) if grounds else np.zeros((0, 4)),
               pred=np.array(pred), post=np.array(post), ml=np.array(ml), has_ml=np.array(has_ml, np.uint8),
               est=np.array(est, np.float64), in_lane=np.array(in_lane, np.uint8))
    return out


def sequences(rng):
    E = (np.zeros(0, np.uint8), np.zeros((0, 4)))
    seqs = {}
    # segments rendered from known lane poses, the robot drifting and turning
    st = []
    for t in range(12):
        d, phi = 0.08 * math.sin(0.5 * t), 0.4 * math.cos(0.3 * t)
        st.append(((0.1, 0.2, 0.3 * math.sin(0.4 * t)), render(rng, d, phi)))
    seqs["poses"] = (DEFAULT, st, None)
    # zero motion: the floors of predict move mass by themselves (row 1 -> 0, columns 2, 4 -> 1, 3)
    seqs["zero_motion"] = (DEFAULT, [((0.0, 0.0, 0.0), render(rng, 0.02, -0.1)) for _ in range(3)] + [((0.1, 0.0, 0.0), E)] * 3, None)
    # v, w != 0: mass leaves the grid
    seqs["leaving"] = (DEFAULT, [((0.5, 0.6, 1.3), render(rng, 0.1, 0.6, n=6)), ((0.5, 0.6, 1.3), E), ((0.4, -0.8, -2.5), E),
                                 ((0.3, 1.0, 3.1), render(rng, -0.05, -0.3, n=6)), ((1.0, 2.0, 4.0), E)], None)
    # frames that do not vote: empty, red only, behind the camera, outside the histogram; then one that does
    red = (np.full(4, 2, np.uint8), render(rng, 0.0, 0.0, n=4)[1])
    c, g = render(rng, 0.0, 0.0, n=4)
    g[:, 0] -= 1.0
    behind = (c, g)
    out_of_grid = render(rng, 0.6, 0.0, n=4)
    steep = render(rng, 0.0, 1.5, n=4)
    good = render(rng, 0.03, 0.2, n=3)
    mixed = tuple(np.concatenate([red[k], behind[k], out_of_grid[k], good[k]]) for k in (0, 1))
    seqs["no_votes"] = (DEFAULT, [((0.1, 0.1, 0.1), E), ((0.1, 0.1, 0.1), red), ((0.1, 0.1, 0.1), behind),
                                  ((0.1, 0.1, 0.1), out_of_grid), ((0.1, 0.1, 0.1), steep), ((0.1, 0.1, 0.1), mixed)], None)
    # the belief concentrated far from the votes: belief * ml sums to 0 and the belief becomes ml
    init = np.zeros((23, 30))
    init[2, 3] = 1.0
    seqs["collapse"] = (DEFAULT, [((0.1, 0.0, 0.0), render(rng, 0.2, 1.1, n=5)), ((0.1, 0.0, 0.0), render(rng, 0.18, 1.0, n=5))], init)
    # a non-default grid (other steps, offsets and blur radii)
    st = []
    for t in range(8):
        d, phi = 0.05 * math.cos(0.7 * t), 0.3 * math.sin(0.5 * t)
        st.append(((0.12, 0.25, -0.4 + 0.1 * t), render(rng, d, phi)))
    seqs["odd_grid"] = (ODD, st, None)
    return seqs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LANE_SLAM_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    warnings.simplefilter("ignore", DeprecationWarning)       # scipy.ndimage.filters, as the reference imports it
    lf = load_reference(ref)
    rng = np.random.default_rng(20261015)
    out = {}
    names = []
    for name, (cfg, steps, init) in sequences(rng).items():
        r = run(lf, cfg, steps, init)
        names.append(name)
        for k, v in r.items():
            out["%s/%s" % (name, k)] = v
    out["names"] = np.array(names)
    path = os.path.join(HERE, "lane_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %s" % (path, ", ".join("%s (%d steps)" % (n, len(out[n + "/dtvw"])) for n in names)))


if __name__ == "__main__":
    main()
