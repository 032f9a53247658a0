"""The designed region-growing images (tests/lsd_grow_cases.py) do what they are for, and the one-lane host build of lsd_grow.h
agrees with the oracle on every one of them.

The first half counts, with the oracle's census (oracle/lf_oracle.h: lfo_lsd_census), what the images make the detector do: how
many of region_grow's decisions fall next to the tolerance, which final sizes the regions have, which parts of the evaluation are
entered.  Each bound is a condition on the inputs, so that a later edit of the generator cannot quietly blunt them; the numbers
obtained stand in the docstring of lsd_grow_cases.py.  The second half keeps the `#else` form of region_grow (tests/hostsim) on the
same inputs the 64-lane form meets in tests/test_gpu_lsd_grow_edges.py."""
import numpy as np
import pytest

import lsd_grow_cases as G
from lane_slam_amd import default_config
from test_hostsim_lsd import _run, hostsim      # noqa: F401  (hostsim is a fixture)

NOTDEF = -1024.0


def _oracle(ang_th=None, seed_order=None, geo="parity"):
    from oracle.oracle import Oracle
    cfg = default_config(geo)
    if ang_th is not None:
        cfg["lsd"]["ang_th"] = ang_th
    if seed_order is not None:
        cfg["lsd"]["seed_order"] = seed_order
    return Oracle(cfg)


def _add(total, c):
    for k, v in c.items():
        if isinstance(v, list):
            total[k] = [a + b for a, b in zip(total.get(k, [0] * len(v)), v)]
        elif k.endswith("_max"):
            total[k] = max(total.get(k, 0), v)
        else:
            total[k] = total.get(k, 0) + v
    return total


def _census(o, cases):
    """({name: lines}, {name: census}, total census) of the cases under the oracle o."""
    lines, per, total = {}, {}, {}
    for name, img in cases:
        lines[name], per[name] = o.lsd(img, census=True)
        _add(total, per[name])
    return lines, per, total


@pytest.fixture(scope="module")
def default_run():
    """Every case a - g under the default parity configuration: the one the device is compared with."""
    return _census(_oracle(), G.all_cases())


@pytest.fixture(scope="module")
def exact_runs():
    return {ang: _census(_oracle(ang_th=ang), G.exact_path_cases()) for ang in G.EXACT_PATH_ANG_TH}


def test_census_off_changes_nothing():
    """The census only counts: the lines with and without it are the same arrays, and a call without it leaves no count behind."""
    o = _oracle()
    for name, img in G.ring_cases()[:2] + [("noise30", G.noise(0.3))]:
        plain = o.lsd(img)
        counted, c = o.lsd(img, census=True)
        assert np.array_equal(plain, counted), name
        assert c["decisions"] > 0
    from oracle.oracle import LsdCensus
    import ctypes
    o.lsd(G.rings(0))
    cs = LsdCensus()
    o.lib.lfo_lsd_census_fetch(ctypes.byref(cs))
    assert cs.as_dict()["decisions"] == 0


def test_cases_are_what_the_generator_says():
    cases = G.all_cases()
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names) and 50 <= len(names) <= 70
    for name, img in cases + G.exact_path_cases():
        assert img.shape == (G.H, G.W) and img.dtype == np.uint8 and set(np.unique(img)) <= {0, 255}, name
    again = dict(G.all_cases())
    assert all(np.array_equal(img, again[name]) for name, img in cases)          # seeded: the same images every time
    assert {n for n, _ in G.exact_path_cases()} <= set(names)


def test_rings_sit_on_the_tolerance(default_run):
    """Over the ring set: at least 100 decisions on each side within 0.0043633 rad of the tolerance (the band in which the 64-lane
    form cannot decide in float), at least 3 on each side within 2e-4 rad, and at least 100 accepted through the 3 pi / 2 fold."""
    _, per, _ = default_run
    t = {}
    for name, _ in G.ring_cases():
        _add(t, per[name])
    print("rings:", t)
    assert t["mid_accepted"] >= 100 and t["mid_rejected"] >= 100
    assert t["near_accepted"] >= 3 and t["near_rejected"] >= 3
    assert t["wrap_accepted"] >= 100


def test_suite_has_decisions_within_2e_4_rad_and_wraps(default_run):
    _, _, t = default_run
    print("all cases:", t)
    assert t["near_accepted"] >= 5 and t["near_rejected"] >= 5
    assert t["wrap_accepted"] >= 100


def test_every_size_bin_is_met(default_run):
    """1, below min_reg_size, min_reg_size itself, up to 63, 64..65 (the first batch of the 64-lane form is full), 66..192, 193..255
    and exactly 256 (the region list's LDS head, LFG_REG_LDS, is nearly full and full), 257 and more (it spills)."""
    _, per, t = default_run
    print("size bins:", t["size_bin"], "max", t["size_max"])
    assert all(n > 0 for n in t["size_bin"]), t["size_bin"]
    assert t["size_max"] > 256
    # the sweeps are what reaches the list's hand-over
    sweep = {}
    for name in per:
        if name.startswith("sweep256"):
            _add(sweep, per[name])
    assert sweep["size_bin"][6] > 0 and sweep["size_bin"][7] > 0 and sweep["size_bin"][8] > 0, sweep["size_bin"]
    # the dashes end on both sides of the threshold: regions of min_reg_size - 1 points (never evaluated) and of min_reg_size
    dash = {}
    for name in ("dashes1", "dashes2", "dashes_vertical"):
        _add(dash, per[name])
    assert dash["size_one_short"] >= 1 and dash["size_bin"][2] >= 1 and dash["size_bin"][3] >= 1, dash


def test_default_is_the_float_path_and_h_the_exact_one(default_run, exact_runs):
    """bulk_ok = prec in (4 * 0.0043633, 0.7).  What is counted is the tolerance of the regions the detector grows from its seeds:
    refine's regrowth takes its tolerance tau from the region's own angles, whatever the configuration is (counted apart; under
    ang_th = 45 most of them land inside the interval)."""
    _, _, t = default_run
    grown = t["seed_prec_inside"] + t["seed_prec_outside"] + t["regrow_prec_inside"] + t["regrow_prec_outside"]
    inside = t["seed_prec_inside"] + t["regrow_prec_inside"]
    print("default: %d of %d regions inside" % (inside, grown))
    assert inside >= 0.95 * grown and t["seed_prec_outside"] == 0
    assert t["regrow_prec_outside"] >= 1               # dotted375: the exact path inside a default image
    for ang, (lines, _, h) in exact_runs.items():
        print("ang_th", ang, h)
        assert h["seed_prec_inside"] == 0 and h["seed_prec_outside"] > 500, ang
        assert sum(len(v) for v in lines.values()) > 8, ang
        assert h["mid_accepted"] >= 10 and h["mid_rejected"] >= 10, ang
    assert exact_runs[0.9][2]["regrow_prec_inside"] == 0


def test_evaluation_paths(default_run):
    """refine entered, a region given up by refine, at least 3 iterations of reduce_region_radius inside one call, every stage of
    rect_improve the one whose rectangle is kept, the first return taken, and the last stage's width guard holding a step back.
    The density rejection is the one path no designed image reached: it comes from the seeded search of
    lsd_grow_cases.search_cases (dotted37, dotted258)."""
    _, per, t = default_run
    print({k: t[k] for k in ("evaluated", "refine_entered", "reduce_iterations", "reduce_iterations_max", "density_rejected",
                             "improve_kept", "improve_reached", "improve_first_return", "improve_last_guard")})
    assert t["refine_entered"] >= 1 and t["density_rejected"] >= 1
    assert t["reduce_iterations_max"] >= 3
    assert all(n >= 1 for n in t["improve_kept"][1:]), t["improve_kept"]
    assert all(n >= 1 for n in t["improve_reached"][1:]), t["improve_reached"]
    assert t["improve_first_return"] >= 1 and t["improve_kept"][0] >= 1
    assert t["improve_last_guard"] >= 1
    assert per["dotted37"]["density_rejected"] + per["dotted258"]["density_rejected"] >= 1
    # without the searched images the designed ones still reach every stage
    designed = {}
    for name in per:
        if not name.startswith("dotted"):
            _add(designed, per[name])
    assert all(n >= 1 for n in designed["improve_kept"][1:]) and designed["reduce_iterations_max"] >= 3
    assert per["zigzag"]["improve_last_guard"] >= 1    # thin rectangles that stop at the last stage's width guard


def test_zigzag_and_many_components(default_run):
    """f: one component whose legs validate, at least 64 of them; g: at least 40 separate components next to a dominant one."""
    lines, _, _ = default_run
    assert G.ZIGZAG_LEGS >= 64 and len(lines["zigzag"]) >= 64
    assert _n_components(G.zigzag()) == 1
    sizes = sorted(_component_sizes(G.many_components()))
    assert len(sizes) == G.N_SHORT_STROKES + 1 >= 41 and sizes[-1] >= 4 * sizes[-2], sizes
    assert len(lines["many_components"]) >= 40


def _component_sizes(img):
    lab = -np.ones(img.shape, np.int64)
    sizes = []
    for y0, x0 in zip(*np.nonzero(img)):
        if lab[y0, x0] >= 0:
            continue
        stack, size = [(y0, x0)], 0
        lab[y0, x0] = len(sizes)
        while stack:
            y, x = stack.pop()
            size += 1
            for yy in range(max(y - 1, 0), min(y + 2, img.shape[0])):
                for xx in range(max(x - 1, 0), min(x + 2, img.shape[1])):
                    if img[yy, xx] and lab[yy, xx] < 0:
                        lab[yy, xx] = len(sizes)
                        stack.append((yy, xx))
        sizes.append(size)
    return sizes


def _n_components(img):
    return len(_component_sizes(img))


def test_tolerance_is_felt():
    """Sensitivity: 0.02 degrees more or less than 22.5 changes the lines of at least one ring image, in each direction -- a margin
    that is off by that much in region_grow cannot hide behind these images."""
    ref = _oracle()
    want = [ref.lsd(img) for _, img in G.ring_cases()]
    for d in (-0.02, 0.02):
        o = _oracle(ang_th=22.5 + d)
        changed = 0
        for (name, img), w in zip(G.ring_cases(), want):
            got = o.lsd(img)
            changed += int(got.shape != w.shape or not np.array_equal(got, w))
        print("ang_th %+.2f: %d of %d ring images change" % (d, changed, len(want)))
        assert changed >= 1, d


def test_composite_is_a_big_problem():
    """Case i has more than 24 000 defined pixels at the fullres geometry: beyond every slice of the row-list kernels."""
    o = _oracle(geo="fullres")
    comp = G.composite()
    assert comp.shape == (320, 640)
    ang, _, order = o.lsd_ll_angle(o.lsd_scaled_image(comp))
    n_def = int((ang != NOTDEF).sum())
    print("composite: %d defined pixels, %d seeds in order, %d lines" % (n_def, len(order), len(o.lsd(comp, cap=8192))))
    assert n_def > 24000 and len(order) > 24000


@pytest.mark.parametrize("by_components", [False, True])
@pytest.mark.parametrize("reg_lds", [0, 37, 1 << 20])
def test_host_form_matches_oracle_on_every_case(hostsim, reg_lds, by_components):
    """lsd_grow.h with one lane: region list fully global / split at 37 / fully "LDS", the problem whole and by components, on
    cases a - g and on the configurations h.  (The harness hands out its seeds in raster order inside a bin, so the oracle it is
    compared with runs that order: tests/test_hostsim_lsd.py.)"""
    total = 0
    for ang, cases in [(None, G.all_cases())] + [(a, G.exact_path_cases()) for a in G.EXACT_PATH_ANG_TH]:
        o = _oracle(ang_th=ang, seed_order="opencv30")
        for name, img in cases:
            ref = o.lsd(img)
            got = _run(hostsim, o, img, reg_lds, by_components=by_components)
            if got.shape != ref.shape or not np.array_equal(got, ref):
                k = next((i for i in range(min(len(got), len(ref))) if not np.array_equal(got[i], ref[i])), min(len(got), len(ref)))
                pytest.fail("%s (ang_th %s, reg_lds %d, by_components %s): %d lines for %d, first difference at line %d: %s / %s"
                            % (name, ang, reg_lds, by_components, len(got), len(ref), k,
                               got[k] if k < len(got) else None, ref[k] if k < len(ref) else None))
            total += len(ref)
    assert total > 2000
