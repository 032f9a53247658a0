"""k_lsd_grow's 64-lane region growing on designed images, at its edges.

The device `region_grow` is not the loop the host simulation runs (tests/test_lsd_grow_cases_cpu.py): a seed window held in lanes,
seven frontier points per batch, a float classification with an exact path for what it cannot decide, de-duplication by ballot,
region lists that start in LDS and go on in global memory.  The images of tests/lsd_grow_cases.py put decisions on the tolerance,
final sizes on every hand-over, strokes on every border and seam; the CPU file proves that from the oracle's census.  Here every
image goes through every form of the kernel -- the bit plane with its default, 64 and 2048 USED bits (64: nearly every case runs
in k_lsd_grow_zl, whose lists are global from the first entry), the row lists at the smallest and the largest slice, in two
launches and in the mixed one -- and must give the oracle's lines, bit for bit and in order, twice on the same handle."""
import os

import numpy as np
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

import lsd_grow_cases as G
from lane_slam_amd import FrontEnd, LanefrontError, default_config

pytestmark = pytest.mark.gpu

NOTDEF = -1024.0
LF_ERR_CAPACITY = -2                                 # include/lanefront.h

# form -> the environment its handle is created under (read once, by lf_create)
FORMS = {
    "bit plane": {},
    "bit plane, 64 USED bits": {"LF_GROW_BITMAP": "64"},
    "bit plane, 2048 USED bits": {"LF_GROW_BITMAP": "2048"},
    "row lists, level 0": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "0", "LF_GROW_MIXED": "0"},
    "row lists, level 2": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "2", "LF_GROW_MIXED": "0"},
    "row lists, mixed launch": {"LF_GROW_BITMAP": "0", "LF_GROW_MIXED": "1"},
}
COMPOSITE_FORMS = {
    "bit plane": {},
    "row lists, level 0": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "0", "LF_GROW_MIXED": "0"},
    "row lists, level 1": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "1", "LF_GROW_MIXED": "0"},
    "row lists, level 2": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "2", "LF_GROW_MIXED": "0"},
    "row lists, level 0, mixed launch": {"LF_GROW_BITMAP": "0", "LF_GROW_LDS_LEVEL": "0", "LF_GROW_MIXED": "1"},
}
_KNOBS = ("LF_GROW_BITMAP", "LF_GROW_LDS_LEVEL", "LF_GROW_MIXED")


def _handle(cfg, env, **kw):
    """A handle created under env; os.environ is as it was afterwards."""
    saved = {k: os.environ.get(k) for k in _KNOBS}
    try:
        for k in _KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return FrontEnd(cfg, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cfg(ang_th=None, geo="parity"):
    cfg = default_config(geo)
    if ang_th is not None:
        cfg["lsd"] = dict(cfg["lsd"], ang_th=ang_th)
    return cfg


@pytest.fixture(scope="module")
def refs():
    """The oracle's lines, once per module: cases a - g under the default configuration, configurations h, the composite."""
    from oracle.oracle import Oracle
    o = Oracle(_cfg())
    out = {None: {name: o.lsd(img) for name, img in G.all_cases()}}
    for ang in G.EXACT_PATH_ANG_TH:
        oh = Oracle(_cfg(ang))
        out[ang] = {name: oh.lsd(img) for name, img in G.exact_path_cases()}
    return out


@pytest.fixture(scope="module")
def composite():
    from oracle.oracle import Oracle
    o = Oracle(_cfg(geo="fullres"))
    img = G.composite()
    ang, _, order = o.lsd_ll_angle(o.lsd_scaled_image(img))
    return img, o.lsd(img, cap=8192), int((ang != NOTDEF).sum()), len(order)


def _difference(name, got, ref):
    """None when got is ref, else one line that says where they part."""
    if got.shape == ref.shape and np.array_equal(got, ref):
        return None
    n = min(len(got), len(ref))
    k = next((i for i in range(n) if not np.array_equal(got[i], ref[i])), n)
    return "%s: %d lines for the oracle's %d, first difference at line %d: device %s, oracle %s" % (
        name, len(got), len(ref), k, got[k].tolist() if k < len(got) else None, ref[k].tolist() if k < len(ref) else None)


def _run_cases(fe, cases, want, tag):
    """Every case, then every case again in the opposite order: the oracle's lines both times (so the second result is the first:
    nothing of an earlier image is left in USED bits, evaluation ring or counters)."""
    bad = []
    first = {}
    for name, img in cases:
        first[name] = fe.lsd_binary(img)
        d = _difference(name, first[name], want[name])
        if d:
            bad.append(d)
    for name, img in reversed(cases):
        again = fe.lsd_binary(img)
        if again.shape != first[name].shape or not np.array_equal(again, first[name]):
            bad.append("%s: the second run on the same handle differs from the first (%s)" % (name, _difference(name, again, want[name])))
    if bad:
        print("\n".join("[%s] %s" % (tag, b) for b in bad))
    assert not bad, "%s: %d of %d cases differ; first: %s" % (tag, len({b.split(":")[0] for b in bad}), len(cases), bad[0])


@pytest.mark.parametrize("form", list(FORMS))
def test_designed_cases_match_oracle_in_every_form(form, refs):
    cases = G.all_cases()
    fe = _handle(_cfg(), FORMS[form], max_frames=1, max_lines_per_color=1024)
    try:
        _run_cases(fe, cases, refs[None], form)
    finally:
        fe.close()
    assert sum(len(v) for v in refs[None].values()) > 1500


@pytest.mark.parametrize("form", ["bit plane", "bit plane, 64 USED bits", "row lists, level 0"])
@pytest.mark.parametrize("ang_th", G.EXACT_PATH_ANG_TH)
def test_exact_path_configurations(ang_th, form, refs):
    """Configurations h: ang_th = 45 (prec >= 0.7) and 0.9 (prec < 4 * 0.0043633) switch the float classification off, every decision
    is the exact one.  A handle of its own each; only the configuration differs."""
    fe = _handle(_cfg(ang_th), FORMS[form], max_frames=1, max_lines_per_color=1024)
    try:
        _run_cases(fe, G.exact_path_cases(), refs[ang_th], "ang_th %g, %s" % (ang_th, form))
    finally:
        fe.close()
    assert sum(len(v) for v in refs[ang_th].values()) > 8


@pytest.mark.parametrize("form", list(COMPOSITE_FORMS))
def test_fullres_composite(form, composite):
    """Case i: more than 24 000 defined pixels, a problem beyond the 13, 28 and 40 KB slices of the row-list kernels alike."""
    img, want, n_def, n_order = composite
    assert n_def > 24000 and n_order > 24000, (n_def, n_order)
    fe = _handle(_cfg(geo="fullres"), COMPOSITE_FORMS[form], max_frames=1, max_lines_per_color=8192)
    try:
        _run_cases(fe, [("composite", img)], {"composite": want}, form)
    finally:
        fe.close()
    assert len(want) > 500


def test_line_capacity_is_exact(refs):
    """A handle with room for exactly the N lines of an image returns all N in order; one with N - 1 says so, and how many."""
    name = "rings1"
    img, want = dict(G.all_cases())[name], refs[None][name]
    n = len(want)
    assert n > 8
    fe = _handle(_cfg(), {}, max_frames=1, max_lines_per_color=n)
    try:
        d = _difference(name, fe.lsd_binary(img), want)
        assert d is None, d
    finally:
        fe.close()
    fe = _handle(_cfg(), {}, max_frames=1, max_lines_per_color=n - 1)
    try:
        with pytest.raises(LanefrontError) as e:
            fe.lsd_binary(img)
        assert e.value.code == LF_ERR_CAPACITY and ("found %d lines" % n) in str(e.value) and ("is %d" % (n - 1)) in str(e.value)
        # and the handle is as good as before: an image that fits
        small = "sloped_bar"
        d = _difference(small, fe.lsd_binary(dict(G.all_cases())[small]), refs[None][small])
        assert d is None, d
    finally:
        fe.close()
