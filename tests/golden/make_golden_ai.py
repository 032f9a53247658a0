#!/usr/bin/env python3
"""Generate tests/golden/anti_instagram.npz: the reference's own AntiInstagram.calculate_transform on camera frames.

Run here only (needs /root/reference and scikit-learn):   python3 tests/golden/make_golden_ai.py
Imported from /root/reference/src/anti_instagram/include/anti_instagram/:
  * kmeans.py          runKMeans / identifyColors / getparameters2 (scikit-learn Lloyd + one lstsq solve)
  * AntiInstagram.py   calculate_transform (the 3- / 4-colour decision, success, health)
Shims: cv2 is stubbed (kmeans.py imports it and never calls it), the duckietown_utils logger is a stub, and
checkMapping's dict.iteritems (Python 2 only) is replaced by a Python 3 equivalent -- its mapping is never read by
getparameters2, so no output depends on it.

Only results are stored, never the frames: the tests rebuild every frame from the committed fixtures with
tests/ai_ref.frames() (real_jpegs.npz decoded by the oracle's JPEG decoder, real_frames.npz, per-channel casts of
those, a synthetic frame that lacks one init colour and a 60-row frame).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src/anti_instagram/include/anti_instagram"

def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference():
    sys.modules["cv2"] = types.ModuleType("cv2")
    du = types.ModuleType("duckietown_utils")
    du.logger = types.SimpleNamespace(info=lambda *a, **k: None)
    sys.modules["duckietown_utils"] = du
    pkg = types.ModuleType("anti_instagram")
    pkg.__path__ = [REF]
    pkg.logger = du.logger
    sys.modules["anti_instagram"] = pkg
    km = _load("anti_instagram.kmeans", os.path.join(REF, "kmeans.py"))

    def checkMapping(mymap):
        maplist, clearmap = [], {}
        for color, mapping in mymap.items():
            if mapping not in maplist:
                clearmap[color] = mapping
                maplist.append(mapping)
        return clearmap
    km.checkMapping = checkMapping
    _load("anti_instagram.scale_and_shift", os.path.join(REF, "scale_and_shift.py"))
    ai = _load("anti_instagram.AntiInstagram", os.path.join(REF, "AntiInstagram.py"))
    return km, ai


def main():
    import contextlib
    import io

    import sklearn
    km, ai = _reference()
    rec = {}
    run0, gp0 = ai.runKMeans, ai.getparameters2

    def runKMeans(img, num_colors, init):
        c, n, s = run0(img, num_colors=num_colors, init=init)
        rec["score%d" % num_colors] = s
        rec["centers%d" % num_colors] = np.array(c, np.float64)
        rec["counts%d" % num_colors] = np.array([n[i] for i in range(num_colors)], np.int64)
        return c, n, s

    def getparameters2(mapping, trained, weights, true):
        r = gp0(mapping, trained, weights, true)
        rec["cost"] = float(np.asarray(r[3]).reshape(-1)[0])
        return r
    ai.runKMeans, ai.getparameters2 = runKMeans, getparameters2

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    import ai_ref
    names, imgs = ai_ref.frames()
    out = {"names": np.array(names), "sklearn_version": np.array(sklearn.__version__)}
    cols = {k: [] for k in ("success", "health", "scale", "shift", "cost", "n_colors", "score3", "score4", "centers", "counts")}
    for img in imgs:
        rec.clear()
        with contextlib.redirect_stdout(io.StringIO()):       # runKMeans prints its timings
            ok, health, par = ai.calculate_transform(img)
        n_colors = 3 if (rec["score3"] + 3e7) > rec["score4"] else 4
        keep = [0, 1, 2] if n_colors == 3 else [0, 2, 3]
        cols["success"].append(bool(ok))
        cols["health"].append(float(health))
        cols["scale"].append(np.asarray(par["scale"], np.float64).reshape(3) if ok else np.zeros(3))
        cols["shift"].append(np.asarray(par["shift"], np.float64).reshape(3) if ok else np.zeros(3))
        cols["cost"].append(rec["cost"])
        cols["n_colors"].append(n_colors)
        cols["score3"].append(float(rec["score3"]))
        cols["score4"].append(float(rec["score4"]))
        cols["centers"].append(rec["centers%d" % n_colors][keep])
        cols["counts"].append(rec["counts%d" % n_colors][keep])
    for k, v in cols.items():
        out[k] = np.array(v)
    np.savez_compressed(os.path.join(HERE, "anti_instagram.npz"), **out)
    print("anti_instagram.npz: %d frames, %d pick 3 colours, %d would publish, scikit-learn %s"
          % (len(names), int(np.sum(out["n_colors"] == 3)), int(np.sum(out["health"] > 0.001)), sklearn.__version__))


if __name__ == "__main__":
    main()
