"""CPU tests of the embedding figures' host side (``figures.py``,
``csrc/figures.hip``): the statistics seaborn's ``kdeplot`` takes from scipy,
restated (covariance, support, density, iso-levels, skipped classes), against
``scipy.stats.gaussian_kde`` and the rule written out here; the refusals of the
three entry points before any HIP call; the step ``figures``.  No kernel is
launched.

Bounds.  Covariance: 1e-12 relative (two products and one power apart from
scipy's).  Support: 4 ulp of the larger end (``lo + i step`` against
``linspace``).  Density: ``|d - ref| <= 1e-9 ref + 1e-12 max(ref)``, the bound
of the device test: a float64 sum of positive terms, the exponent's argument
within 1e-12 relative up to the underflow range (|argument| < 745).
"""
import ctypes
import os

import numpy as np
import pytest

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, evaluation, figures, ops  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def _refused(lib, rc, word, code=-1):
    assert rc == code and word in lib.cfsd_last_error_string(), (rc, lib.cfsd_last_error_string())


def cloud(n, seed):
    """``n`` correlated points with unequal spreads, away from the origin."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 2)) @ np.array([[2.0, 0.0], [1.2, 0.4]]) + np.array([5.0, -3.0])


# ---------------------------------------------------------------- ABI, steps
def test_abi_version_and_constants(lib):
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 23
    for name in ("cfsd_kde2d", "cfsd_density_shade", "cfsd_draw_primitives"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert ops.KDE_CHUNK >= 64 and ops.PRIM_ROUND >= 64 and ops.SHADE_MAX_LEVELS == 8
    assert (ops.PRIM_DISC, ops.PRIM_SEGMENT, ops.PRIM_TRIANGLE) == (0, 1, 2)


def test_steps():
    assert evaluation.Tester.STEPS[:9] == ("traversals", "embeddings", "classifiers", "generation", "metrics",
                                           "interpolate", "tsne", "plan", "prepost")
    assert evaluation.Tester.STEPS[9] == "figures" and len(evaluation.Tester.STEPS) == 10
    for name in ("embedding_figures", "plan_figures", "prepost_figures"):
        assert callable(getattr(evaluation.Tester, name))


def test_class_colours():
    assert [figures.CLASS_COLOURS[c] for c in "nacm"] == ["#ed6e5d", "#74bfc2", "#eecd4a", "#124d81"]
    assert figures.rgb_of("#ed6e5d") == (0xed / 255.0, 0x6e / 255.0, 0x5d / 255.0)
    assert figures.MAIN_SIZE == (480, 640) and figures.GRID == 200


# ---------------------------------------------------------------- statistics against scipy
@pytest.mark.parametrize("n", [3, 17, 130])
def test_kde_statistics_match_scipy(n):
    from scipy.stats import gaussian_kde
    x = cloud(n, n)
    kde = gaussian_kde(x.T, "scott")
    cov = figures.kde_covariance(x)
    np.testing.assert_allclose(cov, kde.covariance, rtol=1e-12, atol=0)
    sd = np.sqrt(np.diag(kde.covariance))
    sup = figures.kde_support(x)
    for a in range(2):
        want = np.linspace(x[:, a].min() - 3 * sd[a], x[:, a].max() + 3 * sd[a], 200)
        got = figures.support_nodes(sup[a, 0], sup[a, 1])
        assert np.abs(got - want).max() <= 4 * EPS * np.abs(want).max(), a
        assert abs(got[0] - want[0]) <= 4 * EPS * abs(want[0]) and abs(got[-1] - want[-1]) <= 4 * EPS * abs(want[-1])
    params = figures.kde_params(x)
    g0, g1 = figures.support_nodes(params[4], params[5]), figures.support_nodes(params[6], params[7])
    # a 41 x 41 sub-grid that keeps the four corners of the support (its farthest tails)
    pick = np.unique(np.concatenate([np.arange(0, 200, 5), [199]]))
    xx, yy = np.meshgrid(g0[pick], g1[pick], indexing="ij")
    ref = kde(np.stack([xx.ravel(), yy.ravel()])).reshape(xx.shape)
    got = figures.density_host(x, params)[np.ix_(pick, pick)]
    err = np.abs(got - ref) - 1e-9 * ref
    print(f"n={n}: density {ref.min():.3e}..{ref.max():.3e}, largest relative error "
          f"{(np.abs(got - ref) / ref).max():.3e}")
    assert ref.min() > 0 and err.max() <= 1e-12 * ref.max()
    # the plain formula, no whitening
    inv, det = np.linalg.inv(kde.covariance), np.linalg.det(kde.covariance)
    d = np.stack([xx.ravel(), yy.ravel()], axis=1)[:, None, :] - x[None]
    plain = np.exp(-0.5 * np.einsum("gki,ij,gkj->gk", d, inv, d)).sum(1) / (n * 2 * np.pi * np.sqrt(det))
    assert (np.abs(got.ravel() - plain) - 1e-9 * plain).max() <= 1e-12 * plain.max()


def rule(values, q):
    """The iso-level rule, written out: sort descending, cumulative share,
    first index whose share reaches 1 - q, clipped to the ends."""
    values = np.asarray(values, dtype=np.float64).ravel()
    order = np.sort(values)[::-1]
    cdf = np.cumsum(order) / values.sum()
    out = []
    for p in q:
        idx = int(np.searchsorted(cdf, 1.0 - p))
        out.append(order[min(max(idx, 0), len(order) - 1)])
    return np.array(out)


def test_iso_levels_follow_the_rule():
    sets = [cloud(n, 7 + n) + shift for n, shift in ((17, 0.0), (40, 1.5), (130, -2.0))]
    grids = [figures.density_host(x, figures.kde_params(x, grid=60), grid=60) for x in sets]
    q5, q68 = figures.iso_proportions(5, 0.05), figures.iso_proportions(1, 0.68)
    assert np.array_equal(q5, np.linspace(0.05, 1, 5)) and np.array_equal(q68, [0.68])
    for g in grids:  # per class
        for q in (q5, q68):
            lv = figures.iso_levels(g, q)
            assert np.array_equal(lv, rule(g, q)) and np.all(np.diff(lv) >= 0)
        lv = figures.iso_levels(g, q5)
        assert lv[-1] == g.max()  # q = 1: the highest node
        for level, q in zip(lv, q5):  # the mass at or above a level reaches 1 - q, and not without the level's nodes
            assert g[g >= level].sum() / g.sum() >= 1 - q - 1e-12
            assert g[g > level].sum() / g.sum() < 1 - q + 1e-12
    share = np.array([len(x) for x in sets], dtype=np.float64) / sum(len(x) for x in sets)
    common = [g * s for g, s in zip(grids, share)]
    for q in (q5, q68):  # common_norm: one set of levels from all grids together
        assert np.array_equal(figures.iso_levels(common, q), rule(np.concatenate([c.ravel() for c in common]), q))
    assert not np.array_equal(figures.iso_levels(common, q5), figures.iso_levels(grids[0], q5))


def test_small_and_collinear_classes_are_skipped():
    t = np.linspace(0.0, 1.0, 9)
    xy = np.concatenate([cloud(20, 1), [[0.0, 0.0], [1.0, 2.0]], np.stack([t, 2.0 * t + 1.0], axis=1), cloud(5, 2)])
    classes = np.array(["n"] * 20 + ["a"] * 2 + ["c"] * 9 + ["m"] * 5)
    kept, skipped = figures.class_sets(xy, classes)
    assert list(kept) == ["n", "m"] and len(kept["n"]) == 20 and len(kept["m"]) == 5
    assert skipped == {"a": "2 points", "c": "singular covariance"}
    assert figures.kde_skip_reason(cloud(3, 3)) is None
    assert figures.kde_skip_reason(np.zeros((4, 2))) == "singular covariance"


def test_marker_primitives_and_pixels():
    panel = {"name": "p", "rect": [10, 20, 100, 50], "window": [0.0, 4.0, -1.0, 1.0]}
    pix = figures.to_pixels(panel, [[0.0, 1.0], [4.0, -1.0], [2.0, 0.0]])
    assert np.array_equal(pix, [[10.0, 20.0], [110.0, 70.0], [60.0, 45.0]])
    layout = {"size": [100, 200], "panels": [panel]}
    rows = figures.marker_primitives(layout, [
        {"panel": "p", "kind": "disc", "xy": [2.0, 0.0], "colour": "#e881a7"},
        {"panel": 0, "kind": "cross", "xy": [2.0, 0.0], "colour": "#e881a7"},
        {"panel": 0, "kind": "arrow", "xy": [0.0, 0.0], "xy2": [4.0, 0.0], "colour": "#a34D7a"},
        {"panel": 0, "kind": "arrow", "xy": [1.0, 0.0], "xy2": [1.0, 0.0], "colour": "#a34D7a"}])  # no length: nothing
    kinds = [int(r[0]) for r in rows]
    assert kinds == [ops.PRIM_DISC, ops.PRIM_SEGMENT, ops.PRIM_SEGMENT, ops.PRIM_SEGMENT, ops.PRIM_TRIANGLE]
    assert all(tuple(r[12:16]) == (10, 20, 110, 70) for r in rows)
    assert tuple(rows[0][1:3]) == (60.0, 45.0) and tuple(rows[4][1:3]) == (110.0, 45.0)  # the head's tip
    with pytest.raises(ValueError, match="kind"):
        figures.marker_primitives(layout, [{"panel": 0, "kind": "star", "xy": [0, 0], "colour": "#000000"}])


def test_unseen_peak_marks_only_classes_below_the_resolution():
    x = cloud(20, 4) * 0.01 + np.array([5.0, 3.0])
    params = figures.kde_params(x)
    grid = figures.density_host(x, params)
    levels = figures.iso_levels(grid, figures.iso_proportions(5, 0.05))
    pi, pj = np.unravel_index(int(np.argmax(grid)), grid.shape)
    peak = [params[4] + pi * params[5], params[6] + pj * params[7]]
    rect = [48, 24, 560, 392]
    far = {"name": "p", "rect": rect, "window": [-1000.0, 1000.0, -600.0, 600.0]}   # the class: 1/100 of a pixel
    near = {"name": "p", "rect": rect, "window": [peak[0] - 0.2, peak[0] + 0.2, peak[1] - 0.1, peak[1] + 0.1]}
    at = figures.unseen_peak(far, params, grid, levels)
    assert at == [int(v) for v in np.floor(figures.to_pixels(far, [peak])[0])]
    assert figures.unseen_peak(near, params, grid, levels) is None
    assert figures.unseen_peak(near, params, grid, levels[:1]) is None           # one level: that level's band
    assert figures.unseen_peak(far, params, grid, levels[:1]) == at
    # the host sample is the kernel's: a pixel centre on a node gives the node, off the support 0
    panel = {"name": "p", "rect": [0, 0, 199, 199], "window": [params[4] - 0.5 * params[5], params[4] + 198.5 * params[5],
                                                               params[6] - 0.5 * params[7], params[6] + 198.5 * params[7]]}
    got = figures.sample_host(panel, params, grid, np.arange(199), np.arange(199))
    assert np.allclose(got, grid[:199, :199][:, ::-1].T, rtol=1e-9, atol=1e-12 * grid.max())
    wide = {"name": "p", "rect": [0, 0, 10, 10], "window": [params[4] - 50.0, params[4] - 40.0, 0.0, 1.0]}
    assert not figures.sample_host(wide, params, grid, np.arange(10), np.arange(10)).any()


# ---------------------------------------------------------------- refusals before any HIP call
def _doubles(rows):
    flat = [float(v) for r in rows for v in r]
    return (ctypes.c_double * len(flat))(*flat)


def _ints(*values):
    return (ctypes.c_int32 * len(values))(*values)


def _floats(rows):
    flat = [float(v) for r in rows for v in r]
    return (ctypes.c_float * len(flat))(*flat)


def test_kde2d_validates_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)
    good = _doubles([[1, 0, 1, 1, 0, 0.1, 0, 0.1]] * 2)

    def call(points=p, set_ptr=_ints(0, 3, 7), params=good, density=p, n=7, s=2, g=200):
        return lib.cfsd_kde2d(points, set_ptr, params, density, n, s, g, None)

    for name in ("points", "set_ptr", "params", "density"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(g=1), b"G=1")
    _refused(lib, call(g=ops.KDE_MAX_G + 1), b"G=")
    _refused(lib, call(s=0), b"bad sizes")
    _refused(lib, call(n=-1), b"bad sizes")
    _refused(lib, call(set_ptr=_ints(0, 5, 3), n=7), b"decreases")
    _refused(lib, call(set_ptr=_ints(0, 3, 8), n=7), b"outside")
    _refused(lib, call(set_ptr=_ints(-1, 3, 7)), b"outside")
    _refused(lib, call(params=_doubles([[1, 0, 1, 1, 0, 0.1, 0, 0.1], [1, 0, 1, 1, 0, 0.0, 0, 0.1]])), b"positive")
    _refused(lib, call(params=_doubles([[1, 0, 1, float("nan"), 0, 0.1, 0, 0.1]] * 2)), b"finite")
    many = 129  # 129 x 4096^2 nodes: past 2^31
    _refused(lib, call(set_ptr=_ints(*range(many + 1)), params=_doubles([[1, 0, 1, 1, 0, 0.1, 0, 0.1]] * many),
                       n=many, s=many, g=4096), b"2^31")


def _panel(px0=0, py0=0, pw=64, ph=48, win=(0.0, 4.0, 0.0, 4.0)):
    return [px0, py0, pw, ph, *win]


def _layer(panel=0, offset=0, g=5, lo=0.0, step=1.0, levels=(0.5,), rgba=(1, 0, 0, 1), fill=1, line=0):
    lv = list(levels) + [0.0] * (8 - min(len(levels), 8))
    return [panel, offset, g, g, lo, step, lo, step, len(levels), *lv[:8], *rgba, fill, line, 0]


def test_density_shade_validates_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)

    def call(image=p, grids=p, panels=(_panel(),), layers=(_layer(),), h=48, w=64, n_panels=None, n_layers=None,
             doubles=25):
        pan = None if panels is None else _doubles(panels)
        lay = None if layers is None else _doubles(layers)
        return lib.cfsd_density_shade(image, grids, pan, lay, h, w, len(panels or ()) if n_panels is None else n_panels,
                                      len(layers or ()) if n_layers is None else n_layers, doubles, None)

    for name in ("image", "grids"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(panels=None, n_panels=1), b"null")
    _refused(lib, call(layers=None, n_layers=1), b"null")
    _refused(lib, call(h=0), b"image")
    _refused(lib, call(panels=[_panel()] * 17), b"17 panels")
    _refused(lib, call(n_layers=0), b"bad sizes")
    _refused(lib, call(panels=(_panel(px0=1),)), b"rectangle outside")          # 1 + 64 > 64
    _refused(lib, call(panels=(_panel(py0=-1),)), b"rectangle outside")
    _refused(lib, call(panels=(_panel(pw=63.5),)), b"rectangle outside")        # not whole pixels
    _refused(lib, call(panels=(_panel(win=(0.0, 0.0, 0.0, 4.0)),)), b"empty window")
    _refused(lib, call(panels=(_panel(pw=40), _panel(px0=32, pw=32))), b"overlap")
    _refused(lib, call(layers=(_layer(panel=1),)), b"no such panel")
    _refused(lib, call(layers=(_layer(levels=[0.1 * k for k in range(9)]),)), b"K=9")
    _refused(lib, call(layers=(_layer(levels=()),)), b"K=0")
    _refused(lib, call(layers=(_layer(g=1),)), b"grid outside")                  # G < 2
    _refused(lib, call(layers=(_layer(offset=1),)), b"grid outside")             # 1 + 25 > 25
    _refused(lib, call(layers=(_layer(step=0.0),)), b"origin / step")
    _refused(lib, call(layers=(_layer(levels=(0.5, 0.4)),)), b"ascending")
    _refused(lib, call(layers=(_layer(rgba=(1, 0, 0, 1.5)),)), b"colour")
    _refused(lib, call(layers=(_layer(fill=2),)), b"flags")


def _disc(x=10, y=10, r=3, rgba=(1, 0, 0, 1), clip=(0, 0, 96, 80), kind=0):
    return [kind, x, y, 0, 0, 0, 0, r, *rgba, *clip]


def test_draw_primitives_validates_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)

    def call(images=p, prims=p, ptr=p, rows=(_disc(), _disc()), host_ptr=_ints(0, 1, 2), b=2, h=80, w=96, n=None):
        host = None if rows is None else _floats(rows)
        return lib.cfsd_draw_primitives(images, prims, ptr, host, host_ptr, b, h, w,
                                        len(rows or ()) if n is None else n, None)

    for name in ("images", "prims", "ptr", "host_ptr"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(rows=None, n=2), b"null")
    _refused(lib, call(w=0), b"image")
    _refused(lib, call(b=0), b"bad sizes")
    _refused(lib, call(b=11, h=8192, w=8192, host_ptr=_ints(0, 1, *[2] * 10)), b"2^31")  # 11 x 3 x 2^26
    _refused(lib, call(host_ptr=_ints(0, 2, 1)), b"decreases")
    _refused(lib, call(host_ptr=_ints(0, 1, 3)), b"outside")
    _refused(lib, call(rows=(_disc(), _disc(kind=3))), b"unknown kind")
    _refused(lib, call(rows=(_disc(x=float("inf")), _disc())), b"finite")
    _refused(lib, call(rows=(_disc(r=-1), _disc())), b"radius")
    _refused(lib, call(rows=(_disc(rgba=(1, 0, 0, 2)), _disc())), b"colour")
    _refused(lib, call(rows=(_disc(), _disc(clip=(0, 0, 97, 80)))), b"clip rectangle outside")
    _refused(lib, call(rows=(_disc(), _disc(clip=(-1, 0, 96, 80)))), b"clip rectangle outside")
    _refused(lib, call(rows=(_disc(), _disc(clip=(0, 0, 96, 81)))), b"clip rectangle outside")
    _refused(lib, call(rows=(_disc(), _disc(clip=(50, 0, 40, 80)))), b"clip rectangle outside")


def test_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        ops.kde2d(torch.zeros(3, 2, dtype=torch.float64), [0, 3], [[1, 0, 1, 1, 0, 0.1, 0, 0.1]], 9)
    with pytest.raises(ValueError, match="device tensor"):
        ops.density_shade(torch.zeros(3, 8, 8), torch.zeros(25, dtype=torch.float64), [_panel(pw=8, ph=8)], [_layer()])
    with pytest.raises(ValueError, match="device tensor"):
        ops.draw_primitives(torch.zeros(1, 3, 8, 8), [_disc(clip=(0, 0, 8, 8))], [0, 1])
