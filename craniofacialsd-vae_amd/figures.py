"""The embedding figures of the reference's ``Tester`` drawn on the device:
class-density maps of a 2-D embedding (``plot_embeddings``,
``plot_embeddings_per_region``, ``test.py:1161-1321``) and point / arrow
overlays on them (``test.py:750-833``, ``1090-1136``).

The reference hands the points to seaborn's ``kdeplot``; seaborn evaluates
scipy's ``gaussian_kde`` (Scott's rule, full covariance) on a 200 x 200 grid
per class, turns iso-proportions into density levels (``_quantile_to_level``)
and lets matplotlib fill between them.  Here the statistics are restated in
NumPy float64 (this file), the densities are evaluated by ``ops.kde2d``, the
bands shaded by ``ops.density_shade`` and the markers composited by
``ops.draw_primitives``.  Nothing is labelled: no font is shipped.  Every
figure comes with the numbers it draws (``figures.json``,
``<prefix>_emb_density.npz``).
"""
import json
import os

import numpy as np
import torch

from . import ops, rendering

GRID = 200          # nodes per axis of a density grid (seaborn's gridsize)
CUT = 3.0           # kernel standard deviations the support reaches past the data (seaborn's cut)
CLASSES = ("n", "a", "c", "m")
CLASS_COLOURS = {"n": "#ed6e5d", "a": "#74bfc2", "c": "#eecd4a", "m": "#124d81"}
PATH_COLOUR, PRE_COLOUR, POST_COLOUR = "#e881a7", "#e881a7", "#a34D7a"
MAIN_SIZE = (480, 640)            # H, W of the main figures
MAIN_PANEL = (48, 24, 560, 392)   # px0, py0, pw, ph
REGION_PANEL = 200                # pixels per region panel, 5 panels per row
REGION_COLUMNS = 5
REGION_MARGIN = 12                # of a region panel, on every side
MARKER_RADIUS, PATH_RADIUS = 2.5, 4.0
FILL_ALPHA, DIST_FILL_ALPHA, DIST_LINE_ALPHA = 0.5, 0.8, 0.5
SINGULAR = 1e-12                  # 1 - correlation^2 at or below this: the class has no 2-D density


def rgb_of(colour):
    """``'#rrggbb'`` -> three floats in [0, 1]."""
    c = colour.lstrip("#")
    if len(c) != 6:
        raise ValueError(f"colour {colour!r}: expected '#rrggbb'")
    return tuple(int(c[i:i + 2], 16) / 255.0 for i in (0, 2, 4))


# ---------------------------------------------------------------- statistics
def kde_covariance(x):
    """Kernel covariance of ``gaussian_kde(x.T, 'scott')``: the data covariance
    (``ddof=1``) times Scott's factor ``n^(-1/6)`` squared."""
    x = np.asarray(x, dtype=np.float64)
    return np.atleast_2d(np.cov(x.T, ddof=1)) * float(len(x)) ** (-1.0 / 3.0)


def kde_skip_reason(x):
    """Why the class with the points ``x`` ``[n, 2]`` gets no density (fewer
    than 3 points, or a singular covariance), or None."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) < 3:
        return f"{len(x)} points"
    c = kde_covariance(x)
    if not np.all(np.isfinite(c)) or c[0, 0] <= 0.0 or c[1, 1] <= 0.0 or \
            c[0, 0] * c[1, 1] - c[0, 1] * c[1, 0] <= SINGULAR * c[0, 0] * c[1, 1]:
        return "singular covariance"
    return None


def kde_support(x, grid=GRID, cut=CUT):
    """Per axis ``(lo, step)`` of ``linspace(min - cut sd, max + cut sd, grid)``,
    ``sd`` the kernel's standard deviation on that axis: ``[2, 2]``."""
    x = np.asarray(x, dtype=np.float64)
    sd = np.sqrt(np.diag(kde_covariance(x)))
    lo, hi = x.min(0) - cut * sd, x.max(0) + cut * sd
    return np.stack([lo, (hi - lo) / (grid - 1)], axis=1)


def support_nodes(lo, step, grid=GRID):
    """The nodes ``lo + i step`` of one axis, as the kernel forms them."""
    return lo + np.arange(grid, dtype=np.float64) * step


def kde_params(x, grid=GRID, cut=CUT):
    """The row of ``ops.kde2d``'s ``params`` for the points ``x`` ``[n, 2]``:
    ``L00, L10, L11`` (Cholesky factor of the inverse kernel covariance),
    ``1 / (n 2 pi sqrt(det))``, ``lo0, step0, lo1, step1``."""
    x = np.asarray(x, dtype=np.float64)
    c = kde_covariance(x)
    low = np.linalg.cholesky(np.linalg.inv(c))
    scale = 1.0 / (len(x) * 2.0 * np.pi * np.sqrt(np.linalg.det(c)))
    sup = kde_support(x, grid, cut)
    return np.array([low[0, 0], low[1, 0], low[1, 1], scale, sup[0, 0], sup[0, 1], sup[1, 0], sup[1, 1]])


def density_host(x, params, grid=GRID):
    """``ops.kde2d`` for one set in NumPy float64 (the whitened sum, in point
    order): ``[grid, grid]``.  For checks on a host without a GPU."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    l00, l10, l11, scale, lo0, st0, lo1, st1 = (float(v) for v in params)
    g0, g1 = support_nodes(lo0, st0, grid)[:, None], support_nodes(lo1, st1, grid)[None, :]
    acc = np.zeros((grid, grid))
    for px, py in x:
        d0, d1 = g0 - px, g1 - py
        u0, u1 = l00 * d0 + l10 * d1, l11 * d1
        acc += np.exp(-0.5 * (u0 * u0 + u1 * u1))
    return scale * acc


def iso_proportions(levels=5, thresh=0.05):
    """seaborn's ``levels=n, thresh=t``: ``linspace(t, 1, n)``."""
    return np.linspace(thresh, 1.0, int(levels))


def iso_levels(grids, q):
    """seaborn's ``_quantile_to_level``: the density levels below which the
    proportions ``q`` of the mass of ``grids`` (one grid, or several taken
    together: ``common_norm``) lie."""
    values = np.concatenate([np.ravel(np.asarray(g, dtype=np.float64)) for g in grids]) \
        if isinstance(grids, (list, tuple)) else np.ravel(np.asarray(grids, dtype=np.float64))
    ordered = np.sort(values)[::-1]
    cdf = np.cumsum(ordered) / values.sum()
    idx = np.searchsorted(cdf, 1.0 - np.asarray(q, dtype=np.float64))
    return np.take(ordered, idx, mode="clip")


def class_sets(xy, classes, order=CLASSES):
    """Per class of ``order`` the rows of ``xy``; classes that get no density
    are reported: ``(kept {class: points}, skipped {class: reason})``."""
    xy, classes = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(classes)
    kept, skipped = {}, {}
    for c in order:
        pts = xy[classes == c]
        why = kde_skip_reason(pts)
        if why is None:
            kept[c] = pts
        elif len(pts):
            skipped[c] = why
    return kept, skipped


# ---------------------------------------------------------------- layout
def _window(arrays, margin=0.05):
    """Data window ``[xlo, xhi, ylo, yhi]`` holding every ``[n, 2]`` array, widened by ``margin`` per side."""
    arrays = [np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in arrays if len(a)]
    if not arrays:
        return [0.0, 1.0, 0.0, 1.0]
    pts = np.concatenate(arrays)
    lo, hi = pts.min(0), pts.max(0)
    pad = np.where(hi > lo, (hi - lo) * margin, 1.0)
    return [float(lo[0] - pad[0]), float(hi[0] + pad[0]), float(lo[1] - pad[1]), float(hi[1] + pad[1])]


def _support_corners(params):
    p = np.asarray(params, dtype=np.float64).reshape(-1, 8)
    return [np.array([[r[4], r[6]], [r[4] + (GRID - 1) * r[5], r[6] + (GRID - 1) * r[7]]]) for r in p]


def to_pixels(panel, xy):
    """Data coordinates -> pixel coordinates of ``panel`` (``{"rect", "window"}``)."""
    px0, py0, pw, ph = panel["rect"]
    xlo, xhi, ylo, yhi = panel["window"]
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.stack([px0 + (xy[:, 0] - xlo) / (xhi - xlo) * pw, py0 + (yhi - xy[:, 1]) / (yhi - ylo) * ph], axis=1)


def _prim(kind, geom, r, colour, alpha, clip):
    row = np.zeros(ops.PRIM_FLOATS, dtype=np.float32)
    row[0] = kind
    row[1:1 + len(geom)] = geom
    row[7] = r
    row[8:11] = rgb_of(colour) if isinstance(colour, str) else colour
    row[11] = alpha
    row[12:16] = clip
    return row


def _clip_of(rect):
    return (rect[0], rect[1], rect[0] + rect[2], rect[1] + rect[3])


def disc(p, r, colour, clip, alpha=1.0):
    return [_prim(ops.PRIM_DISC, [p[0], p[1]], r, colour, alpha, clip)]


def cross(p, r, colour, clip, alpha=1.0):
    return [_prim(ops.PRIM_SEGMENT, [p[0] - r, p[1] - r, p[0] + r, p[1] + r], 0.5, colour, alpha, clip),
            _prim(ops.PRIM_SEGMENT, [p[0] - r, p[1] + r, p[0] + r, p[1] - r], 0.5, colour, alpha, clip)]


def arrow(a, b, colour, clip, head=9.0, half=4.0, alpha=1.0):
    """A segment from ``a`` to ``b`` and a triangular head at ``b`` (pixels)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    length = float(np.hypot(*(b - a)))
    if length == 0.0:
        return []
    d = (b - a) / length
    n = np.array([-d[1], d[0]])
    base = b - d * min(head, length)
    return [_prim(ops.PRIM_SEGMENT, [a[0], a[1], base[0], base[1]], 0.75, colour, alpha, clip),
            _prim(ops.PRIM_TRIANGLE, [b[0], b[1], base[0] + n[0] * half, base[1] + n[1] * half,
                                      base[0] - n[0] * half, base[1] - n[1] * half], 0.0, colour, alpha, clip)]


def _frame(rect, size):
    """The four sides of a panel's frame."""
    x0, y0, x1, y1 = _clip_of(rect)
    full = (0, 0, size[1], size[0])
    sides = [(x0, y0, x1, y0), (x0, y1, x1, y1), (x0, y0, x0, y1), (x1, y0, x1, y1)]
    return [_prim(ops.PRIM_SEGMENT, s, 0.5, (0.0, 0.0, 0.0), 1.0, full) for s in sides]


def _legend(x, y, size, colours, length=14.0, half=3.0):
    """A strip of colour swatches, one per class, from ``(x, y)`` to the right."""
    full = (0, 0, size[1], size[0])
    pitch = length + 2.0 * half + 2.0
    return [_prim(ops.PRIM_SEGMENT, [x + pitch * k, y, x + length + pitch * k, y], half, c, 1.0, full)
            for k, c in enumerate(colours)]


def _draw(image, prims):
    if prims:
        ops.draw_primitives(image.unsqueeze(0), np.stack(prims), [0, len(prims)])
    return image


def _layer(panel, offset, params, levels, colour, alpha, fill, line):
    row = np.zeros(ops.SHADE_LAYER_DOUBLES)
    row[0], row[1], row[2], row[3] = panel, offset, GRID, GRID
    row[4:8] = params[4:8]
    row[8] = len(levels)
    row[9:9 + len(levels)] = levels
    row[17:20] = rgb_of(colour)
    row[20], row[21], row[22] = alpha, float(fill), float(line)
    return row


def _panel_row(panel):
    return list(panel["rect"]) + list(panel["window"])


def _scatter(panel, xy, classes, crossed, order=CLASSES):
    """Discs (crosses where ``crossed``) of the rows in class order."""
    clip, out = _clip_of(panel["rect"]), []
    pix = to_pixels(panel, xy)
    for c in order:
        for k in np.flatnonzero(np.asarray(classes) == c):
            out += (cross if crossed[k] else disc)(pix[k], MARKER_RADIUS, CLASS_COLOURS[c], clip)
    return out


def sample_host(panel, params, grid, xs, ys):
    """``ops.density_shade``'s sample of ``grid`` ``[G, G]`` (``params``: its
    ``kde_params`` row) at the centres of the pixels ``xs`` x ``ys`` of
    ``panel``, in NumPy float64 with the operations of ``include/cfsd.h`` in
    their order: ``[len(ys), len(xs)]``, 0 outside the grid's support."""
    px0, py0, pw, ph = (float(v) for v in panel["rect"])
    xlo, xhi, ylo, yhi = (float(v) for v in panel["window"])
    g0, g1 = grid.shape
    x = np.asarray(xs, dtype=np.float64)[None, :]
    y = np.asarray(ys, dtype=np.float64)[:, None]
    dx, dy = xlo + (x + 0.5 - px0) / pw * (xhi - xlo), yhi - (y + 0.5 - py0) / ph * (yhi - ylo)
    u, v = np.broadcast_arrays((dx - params[4]) / params[5], (dy - params[6]) / params[7])
    inside = (u >= 0) & (u <= g0 - 1) & (v >= 0) & (v <= g1 - 1)
    i0 = np.minimum(np.where(inside, u, 0).astype(np.int64), g0 - 2)
    j0 = np.minimum(np.where(inside, v, 0).astype(np.int64), g1 - 2)
    fu, fv = u - i0, v - j0
    a = grid[i0, j0] * (1.0 - fu) + grid[i0 + 1, j0] * fu
    b = grid[i0, j0 + 1] * (1.0 - fu) + grid[i0 + 1, j0 + 1] * fu
    return np.where(inside, a * (1.0 - fv) + b * fv, 0.0)


UNSEEN_MAX_PIXELS = 4096  # a top band whose box holds more pixel centres than this is taken to hold one


def unseen_peak(panel, params, grid, levels):
    """The pixel ``[x, y]`` of ``panel`` that holds the highest node of
    ``grid``, when no pixel centre of the panel lies in the top band of
    ``levels`` (the density at or above ``levels[max(K - 2, 0)]``, the band
    drawn in the pure colour) -- a class tighter than the picture's resolution,
    of which ``ops.density_shade``, sampling at pixel centres, draws nothing
    there; else None.  matplotlib strokes such a contour with its line width;
    here :func:`embedding_figures` paints that one pixel."""
    grid = np.asarray(grid, dtype=np.float64)
    top = float(levels[max(len(levels) - 2, 0)])
    i, j = np.nonzero(grid >= top)
    if not len(i):
        return None
    px0, py0, pw, ph = panel["rect"]
    g = grid.shape[0]
    # the box of the band's nodes, one node wider on every side, in pixels (rows grow downwards)
    lo = [params[4] + (max(i.min() - 1, 0)) * params[5], params[6] + (max(j.min() - 1, 0)) * params[7]]
    hi = [params[4] + (min(i.max() + 1, g - 1)) * params[5], params[6] + (min(j.max() + 1, g - 1)) * params[7]]
    (x0, y1), (x1, y0) = to_pixels(panel, [lo, hi])
    xs = np.arange(max(int(np.ceil(x0 - 0.5)), px0), min(int(np.floor(x1 - 0.5)), px0 + pw - 1) + 1)
    ys = np.arange(max(int(np.ceil(y0 - 0.5)), py0), min(int(np.floor(y1 - 0.5)), py0 + ph - 1) + 1)
    if len(xs) * len(ys) > UNSEEN_MAX_PIXELS:
        return None
    if len(xs) and len(ys) and (sample_host(panel, params, grid, xs, ys) >= top).any():
        return None
    pi, pj = np.unravel_index(int(np.argmax(grid)), grid.shape)
    x, y = to_pixels(panel, [[params[4] + pi * params[5], params[6] + pj * params[7]]])[0]
    return [int(min(max(np.floor(x), px0), px0 + pw - 1)), int(min(max(np.floor(y), py0), py0 + ph - 1))]


def _peak_marks(panel, sets, owner, params, grids, levels, alpha):
    """Per class of ``sets`` whose top band no pixel centre sees: the pixel of its peak, and the primitive that
    paints exactly that pixel (a disc of radius 1/2 on the pixel's centre covers it and no neighbour)."""
    marked, prims = {}, []
    for s in sets:
        c = owner[s][1]
        at = unseen_peak(panel, params[s], grids[s], levels[c])
        if at is not None:
            marked[c] = at
            prims += disc((at[0] + 0.5, at[1] + 0.5), 0.5, CLASS_COLOURS[c], _clip_of(panel["rect"]), alpha)
    return marked, prims


def _blank(size, device):
    return torch.ones((3, size[0], size[1]), dtype=torch.float32, device=device)


# ---------------------------------------------------------------- the figures
def embedding_figures(xy, classes, is_test, augmented, out_dir, prefix="lda", regions=None, device="cuda"):
    """Draw the figures of ``plot_embeddings`` for the 2-D embedding ``xy``
    ``[N, 2]`` with per row its class letter, ``is_test`` and ``augmented``:

    ``<prefix>_emb_train_vs_test.png`` (discs: train, crosses: test),
    ``<prefix>_emb_real_vs_aug.png`` (discs: real, crosses: augmented),
    ``<prefix>_emb_real_dist_vs_sc_aug.png`` (common-norm filled bands of the
    real training rows, the augmented rows scattered) and
    ``<prefix>_emb_distributions.png`` (per-class filled bands and lines), all
    640 x 480; with ``regions`` ``{name: [N_train, 2]}`` (the training rows'
    per-region embeddings) ``emb_all_train.png`` and ``emb_all_train_dist.png``,
    five 200-pixel panels per row, real rows only, one 0.68 line per class.

    ``ops.density_shade`` samples at pixel centres, so of a class whose top band
    holds no pixel centre it draws nothing there; such a class gets the one
    pixel that holds its density peak painted in its colour
    (:func:`unseen_peak`) and is listed under ``marked``.

    Writes ``figures.json`` (per file the panels, windows, colours, levels,
    skipped and marked classes) and ``<prefix>_emb_density.npz`` (grids, supports).
    Returns ``{key: {"path", "image" [3, H, W] (device), "layout"}}`` with the
    keys ``train_vs_test, real_vs_aug, real_dist_vs_sc_aug, distributions,
    all_train, all_train_dist``, for :func:`overlay`."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    classes, is_test, augmented = np.asarray(classes), np.asarray(is_test, bool), np.asarray(augmented, bool)
    if not (len(xy) == len(classes) == len(is_test) == len(augmented)) or not len(xy):
        raise ValueError("xy, classes, is_test and augmented must name the same (non-empty) rows")
    os.makedirs(out_dir, exist_ok=True)
    order = [c for c in CLASSES if np.any(classes == c)] + sorted(set(classes.tolist()) - set(CLASSES))
    unknown = [c for c in order if c not in CLASS_COLOURS]
    if unknown:
        raise ValueError(f"classes {unknown} have no colour (known: {list(CLASS_COLOURS)})")
    real_train = ~is_test & ~augmented
    region_items = list(regions.items()) if regions else []
    train_classes, train_real = classes[~is_test], ~augmented[~is_test]
    for name, e in region_items:
        if np.asarray(e).shape != (int((~is_test).sum()), 2):
            raise ValueError(f"region {name!r}: shape {np.asarray(e).shape}, expected one [x1, x2] per training row")

    # every density of the figure set in one launch: the classes of the main embedding, then of each region
    groups = [("main", *class_sets(xy[real_train], classes[real_train], order))]
    for name, e in region_items:
        groups.append((str(name), *class_sets(np.asarray(e, dtype=np.float64)[train_real], train_classes[train_real],
                                              order)))
    points, set_ptr, params, owner = [], [0], [], []
    for g, (_, kept, _) in enumerate(groups):
        for c, pts in kept.items():
            points.append(pts)
            set_ptr.append(set_ptr[-1] + len(pts))
            params.append(kde_params(pts))
            owner.append((g, c))
    params = np.array(params).reshape(-1, 8)
    if owner:
        d_density = ops.kde2d(torch.from_numpy(np.concatenate(points)).to(device).contiguous(), set_ptr, params, GRID)
        density = d_density.cpu().numpy()
    else:
        d_density, density = None, np.zeros((0, GRID, GRID))
    rows_of = [int(real_train.sum())] + [int(train_real.sum())] * len(region_items)  # skipped classes included
    share = np.array([(set_ptr[s + 1] - set_ptr[s]) / rows_of[g] for s, (g, _) in enumerate(owner)])
    common = density * share[:, None, None]  # common_norm: each class's density by its share of the rows
    if owner:
        d_common = (d_density * torch.from_numpy(share).to(device)[:, None, None]).contiguous()
        d_grids = torch.cat([d_density.reshape(-1), d_common.reshape(-1)])
    cells = GRID * GRID
    main_sets = [s for s, (g, _) in enumerate(owner) if g == 0]

    def levels_of(sets, q, together):
        if together:
            lv = iso_levels([common[s] for s in sets], q) if sets else np.zeros(0)
            return {owner[s][1]: lv for s in sets}
        return {owner[s][1]: iso_levels(density[s], q) for s in sets}

    size = MAIN_SIZE
    window = _window([xy] + [c for s in main_sets for c in _support_corners(params[s])])
    main_panel = {"name": prefix, "rect": list(MAIN_PANEL), "window": window}
    out, sidecar = {}, {}

    def finish(key, fname, image, panels, prims, levels=None, skipped=None, size=size, marked=None):
        swatches = [CLASS_COLOURS[c] for c in order]
        # every panel gets its frame and its legend strip: under a main panel, in the margin above a region panel
        for p in panels:
            prims = prims + _frame(p["rect"], size)
            if size == MAIN_SIZE:
                prims = prims + _legend(p["rect"][0] + 4.0, p["rect"][1] + p["rect"][3] + 16.0, size, swatches)
            else:
                prims = prims + _legend(p["rect"][0] + 3.0, p["rect"][1] - 6.0, size, swatches, length=8.0, half=2.0)
        _draw(image, prims)
        path = rendering.save_png(os.path.join(out_dir, fname), image)
        layout = {"size": list(size), "panels": panels}
        out[key] = {"path": path, "image": image, "layout": layout}
        sidecar[fname] = {"size": list(size), "panels": panels, "colours": {c: CLASS_COLOURS[c] for c in order},
                          "levels": levels or {}, "skipped": skipped or {}, "marked": marked or {}}

    finish("train_vs_test", f"{prefix}_emb_train_vs_test.png", _blank(size, device), [main_panel],
           _scatter(main_panel, xy, classes, is_test, order))
    finish("real_vs_aug", f"{prefix}_emb_real_vs_aug.png", _blank(size, device), [main_panel],
           _scatter(main_panel, xy, classes, augmented, order))

    q5 = iso_proportions(5, 0.05)
    skipped_main = groups[0][2]
    image = _blank(size, device)
    lv = levels_of(main_sets, q5, together=True)
    layers = [_layer(0, (len(owner) + s) * cells, params[s], lv[owner[s][1]], CLASS_COLOURS[owner[s][1]], FILL_ALPHA,
                     True, False) for s in main_sets]
    if layers:
        ops.density_shade(image, d_grids, [_panel_row(main_panel)], layers)
    aug = augmented & ~is_test
    marked, marks = _peak_marks(main_panel, main_sets, owner, params, common, lv, FILL_ALPHA)
    finish("real_dist_vs_sc_aug", f"{prefix}_emb_real_dist_vs_sc_aug.png", image, [main_panel],
           marks + _scatter(main_panel, xy[aug], classes[aug], np.zeros(int(aug.sum()), bool), order),
           {prefix: {c: v.tolist() for c, v in lv.items()}}, {prefix: skipped_main}, marked={prefix: marked})

    image = _blank(size, device)
    lv = levels_of(main_sets, q5, together=False)
    layers = []
    for s in main_sets:
        c = owner[s][1]
        layers.append(_layer(0, s * cells, params[s], lv[c], CLASS_COLOURS[c], DIST_FILL_ALPHA, True, False))
        layers.append(_layer(0, s * cells, params[s], lv[c], CLASS_COLOURS[c], DIST_LINE_ALPHA, False, True))
    if layers:
        ops.density_shade(image, d_grids, [_panel_row(main_panel)], layers)
    marked, marks = _peak_marks(main_panel, main_sets, owner, params, density, lv, DIST_FILL_ALPHA)
    finish("distributions", f"{prefix}_emb_distributions.png", image, [main_panel], marks,
           {prefix: {c: v.tolist() for c, v in lv.items()}}, {prefix: skipped_main}, marked={prefix: marked})

    if region_items:
        rows = (len(region_items) + REGION_COLUMNS - 1) // REGION_COLUMNS
        rsize = (rows * REGION_PANEL, REGION_COLUMNS * REGION_PANEL)
        side = REGION_PANEL - 2 * REGION_MARGIN
        panels = []
        for r, (name, e) in enumerate(region_items):
            e = np.asarray(e, dtype=np.float64)[train_real]
            sets = [s for s, (g, _) in enumerate(owner) if g == r + 1]
            rect = [(r % REGION_COLUMNS) * REGION_PANEL + REGION_MARGIN,
                    (r // REGION_COLUMNS) * REGION_PANEL + REGION_MARGIN, side, side]
            panels.append({"name": str(name), "rect": rect,
                           "window": _window([e] + [c for s in sets for c in _support_corners(params[s])])})
        prims = []
        for p, (name, e) in zip(panels, region_items):
            e = np.asarray(e, dtype=np.float64)[train_real]
            prims += _scatter(p, e, train_classes[train_real], np.zeros(len(e), bool), order)
        finish("all_train", "emb_all_train.png", _blank(rsize, device), panels, prims, size=rsize)
        image, q68, levels, skipped = _blank(rsize, device), iso_proportions(1, 0.68), {}, {}
        marked, marks = {}, []
        for p0 in range(0, len(panels), ops.SHADE_MAX_PANELS):
            layers = []
            for r in range(p0, min(p0 + ops.SHADE_MAX_PANELS, len(panels))):
                sets = [s for s, (g, _) in enumerate(owner) if g == r + 1]
                lv = levels_of(sets, q68, together=True)
                levels[panels[r]["name"]] = {c: v.tolist() for c, v in lv.items()}
                skipped[panels[r]["name"]] = groups[r + 1][2]
                marked[panels[r]["name"]], more = _peak_marks(panels[r], sets, owner, params, common, lv, 1.0)
                marks += more
                layers += [_layer(r - p0, (len(owner) + s) * cells, params[s], lv[owner[s][1]],
                                  CLASS_COLOURS[owner[s][1]], 1.0, False, True) for s in sets]
            if layers:
                ops.density_shade(image, d_grids, [_panel_row(p) for p in panels[p0:p0 + ops.SHADE_MAX_PANELS]],
                                  layers)
        finish("all_train_dist", "emb_all_train_dist.png", image, panels, marks, levels, skipped, size=rsize,
               marked=marked)

    listed = {}
    if os.path.exists(os.path.join(out_dir, "figures.json")):  # the figures of another prefix stay listed
        with open(os.path.join(out_dir, "figures.json")) as f:
            listed = json.load(f)
    with open(os.path.join(out_dir, "figures.json"), "w") as f:
        json.dump({**listed, **sidecar}, f, indent=1)
    np.savez(os.path.join(out_dir, f"{prefix}_emb_density.npz"), density=density, share=share, params=params,
             set_ptr=np.array(set_ptr), group=np.array([groups[g][0] for g, _ in owner]),
             **{"class": np.array([c for _, c in owner])},
             support=np.stack([np.stack([support_nodes(p[4], p[5]), support_nodes(p[6], p[7])]) for p in params])
             if len(params) else np.zeros((0, 2, GRID)))
    return out


def marker_primitives(layout, markers):
    """Primitive rows of ``markers`` on the panels of ``layout``: each marker a
    dict with ``panel`` (name or index), ``kind`` (``disc``, ``cross`` or
    ``arrow``), ``xy`` (``arrow``: also ``xy2``) in data coordinates,
    ``colour`` and optionally ``radius`` (pixels) and ``alpha``.  A marker is
    clipped to its panel."""
    names = {p["name"]: p for p in layout["panels"]}
    rows = []
    for m in markers:
        panel = names[m["panel"]] if m["panel"] in names else layout["panels"][m["panel"]]
        clip, alpha = _clip_of(panel["rect"]), float(m.get("alpha", 1.0))
        p = to_pixels(panel, m["xy"])[0]
        if m["kind"] == "disc":
            rows += disc(p, float(m.get("radius", PATH_RADIUS)), m["colour"], clip, alpha)
        elif m["kind"] == "cross":
            rows += cross(p, float(m.get("radius", PATH_RADIUS)), m["colour"], clip, alpha)
        elif m["kind"] == "arrow":
            rows += arrow(p, to_pixels(panel, m["xy2"])[0], m["colour"], clip, alpha=alpha)
        else:
            raise ValueError(f"marker kind {m['kind']!r}: expected disc, cross or arrow")
    return rows


def overlay(base, layout, frames):
    """``B = len(frames)`` copies of the figure ``base`` ``[3, H, W]`` with the
    markers of each frame (:func:`marker_primitives`) drawn on its copy, all in
    one ``ops.draw_primitives`` launch: ``[B, 3, H, W]``."""
    if base.dim() != 3 or base.shape[0] != 3 or not len(frames):
        raise ValueError(f"base {tuple(base.shape)} / {len(frames)} frames: expected [3, H, W] and at least one frame")
    images = base.unsqueeze(0).repeat(len(frames), 1, 1, 1).contiguous()
    rows, ptr = [], [0]
    for markers in frames:
        rows += marker_primitives(layout, markers)
        ptr.append(len(rows))
    if rows:
        ops.draw_primitives(images, np.stack(rows), ptr)
    return images
