"""The embedding figures on the GPU (``csrc/figures.hip``, ``figures.py``,
``evaluation.py``; reference ``test.py:750-833``, ``1090-1136``, ``1161-1321``).

References.  ``kde2d``: ``scipy.stats.gaussian_kde`` (Scott's rule) in float64;
a set of one point, for which scipy has no covariance, the plain formula.
``density_shade``: the NumPy float64 / fp32 restatement below, operation for
operation as ``include/cfsd.h`` states them.  ``draw_primitives``: the NumPy
fp32 restatement below.  End to end: the host rule of ``figures.py`` applied to
the grids the run saved, and the restatements replayed on the run's own layout.

Bounds.  ``kde2d``: ``|d - ref| <= 1e-9 ref + 1e-12 max(ref)`` -- all terms are
positive, so a sequential float64 sum of <= 4096 terms is within 4.5e-13
relative, and the exponent's argument stays within 1e-12 relative up to the
underflow range.  ``density_shade``: equal bit for bit (grids of small integers,
levels at k + 1/3 that no sample attains, nothing fused on either side, IEEE
division and multiplication on both).  ``draw_primitives``: 1e-4 (coordinates
are multiples of 1/8 pixel, so differences are exact; what remains is the
rounding of sqrt and of fused multiply-adds near an edge, about 4 ulp of 16 =
4e-6 per primitive, over at most 8 blends); a pixel farther than r + 1/2 from
every primitive equals the input bit for bit.
"""
import json
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe

pytestmark = pytest.mark.gpu
cfsd_loader.load()
from craniofacialsd_vae_amd import evaluation, figures, ops  # noqa: E402
from test_evaluation_host import check_apng  # noqa: E402
from test_render_host import decode_png  # noqa: E402

DEV = "cuda"
C = ops.KDE_CHUNK
F32 = np.float32


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 2)) @ np.array([[2.0, 0.0], [1.2, 0.4]]) + np.array([5.0, -3.0])


# ---------------------------------------------------------------- kde2d
SIZES = (0, 1, 3, C - 1, C, C + 1, 2 * C + 7)
LONE = [1.3, -0.4, 0.8, 0.37, -2.0, 0.5, 1.0, 0.25]  # parameters of the sets scipy has no covariance for


def kde_problem(grid):
    sets = [cloud(n, 11 + n) for n in SIZES]
    params = np.array([figures.kde_params(x, grid=grid) if len(x) >= 3 else LONE for x in sets])
    set_ptr = np.concatenate([[0], np.cumsum([len(x) for x in sets])])
    return sets, params, set_ptr


def kde_reference(x, params, grid):
    from scipy.stats import gaussian_kde
    g0, g1 = figures.support_nodes(params[4], params[5], grid), figures.support_nodes(params[6], params[7], grid)
    xx, yy = np.meshgrid(g0, g1, indexing="ij")
    if len(x) == 0:
        return np.zeros((grid, grid))
    if len(x) < 3:  # the plain formula
        low = np.array([[params[0], 0.0], [params[1], params[2]]])
        d = np.stack([xx.ravel(), yy.ravel()], axis=1)[:, None, :] - x[None]
        u = d @ low  # rows: (L^T d)^T = d^T L
        return (params[3] * np.exp(-0.5 * (u ** 2).sum(-1)).sum(1)).reshape(grid, grid)
    return gaussian_kde(x.T, "scott")(np.stack([xx.ravel(), yy.ravel()])).reshape(grid, grid)


def check_density(got, ref, what):
    excess = np.abs(got - ref) - 1e-9 * ref
    rel = (np.abs(got - ref) / np.where(ref > 0, ref, 1.0)).max()
    print(f"{what}: density {ref.min():.3e}..{ref.max():.3e}, largest relative error {rel:.3e}, "
          f"excess over 1e-9 ref {excess.max():.3e} (bound {1e-12 * ref.max():.3e})")
    assert excess.max() <= 1e-12 * ref.max(), what


@pytest.mark.parametrize("grid", [9, 33])
def test_kde2d_vs_scipy(grid):
    sets, params, set_ptr = kde_problem(grid)
    points = torch.from_numpy(np.concatenate(sets)).to(DEV)
    got = ops.kde2d(points, set_ptr, params, grid)
    assert got.shape == (len(SIZES), grid, grid) and got.dtype == torch.float64
    again = ops.kde2d(points, set_ptr, params, grid)
    assert torch.equal(got, again)  # two calls, equal bits
    host = got.cpu().numpy()
    assert not host[0].any()  # the empty set
    for s, x in enumerate(sets):
        check_density(host[s], kde_reference(x, params[s], grid), f"G={grid} set of {len(x)}")
        if len(x):  # the set alone, at another place in the point array
            alone = ops.kde2d(torch.from_numpy(x).to(DEV), [0, len(x)], params[s:s + 1], grid)
            assert torch.equal(alone[0], got[s]), len(x)
    empty = ops.kde2d(points[:0].contiguous(), [0, 0], params[:1], grid)
    assert not empty.cpu().numpy().any()


def test_kde2d_full_grid():
    x = cloud(130, 5)
    params = figures.kde_params(x)
    got = ops.kde2d(torch.from_numpy(x).to(DEV), [0, 130], params[None], figures.GRID)[0].cpu().numpy()
    check_density(got, kde_reference(x, params, figures.GRID), "G=200, 130 points")
    check_density(got, figures.density_host(x, params), "G=200 against the host fallback")


def test_kde2d_many_sets_cross_launch_groups():
    """More sets than one launch carries: every set still equals its own call."""
    sets = [cloud(3 + s % 5, 100 + s) for s in range(37)]
    params = np.array([figures.kde_params(x, grid=9) for x in sets])
    set_ptr = np.concatenate([[0], np.cumsum([len(x) for x in sets])])
    got = ops.kde2d(torch.from_numpy(np.concatenate(sets)).to(DEV), set_ptr, params, 9)
    for s in (0, 31, 32, 36):
        alone = ops.kde2d(torch.from_numpy(sets[s]).to(DEV), [0, len(sets[s])], params[s:s + 1], 9)
        assert torch.equal(alone[0], got[s]), s


# ---------------------------------------------------------------- density_shade
def bands_of(panel, layer, grids):
    """Bands of every pixel of the panel: [ph, pw] int, float64, the operations of cfsd.h in their order."""
    px0, py0, pw, ph, xlo, xhi, ylo, yhi = (float(v) for v in panel)
    off, g0, g1 = int(layer[1]), int(layer[2]), int(layer[3])
    lo0, st0, lo1, st1 = (float(v) for v in layer[4:8])
    k = int(layer[8])
    x = np.arange(int(px0), int(px0 + pw), dtype=np.float64)[None, :]
    y = np.arange(int(py0), int(py0 + ph), dtype=np.float64)[:, None]
    tx, ty = (x + 0.5 - px0) / pw, (y + 0.5 - py0) / ph
    dx, dy = xlo + tx * (xhi - xlo), yhi - ty * (yhi - ylo)
    u, v = np.broadcast_arrays((dx - lo0) / st0, (dy - lo1) / st1)
    inside = (u >= 0) & (u <= g0 - 1) & (v >= 0) & (v <= g1 - 1)
    i0 = np.minimum(np.where(inside, u, 0).astype(np.int64), g0 - 2)
    j0 = np.minimum(np.where(inside, v, 0).astype(np.int64), g1 - 2)
    fu, fv = u - i0, v - j0
    g = np.asarray(grids[off:off + g0 * g1], dtype=np.float64).reshape(g0, g1)
    a = g[i0, j0] * (1.0 - fu) + g[i0 + 1, j0] * fu
    b = g[i0, j0 + 1] * (1.0 - fu) + g[i0 + 1, j0 + 1] * fu
    d = np.where(inside, a * (1.0 - fv) + b * fv, 0.0)
    return (np.asarray(layer[9:9 + k], dtype=np.float64)[:, None, None] <= d[None]).sum(0), d


def shade_reference(image, grids, panels, layers):
    """``ops.density_shade`` in NumPy: float64 sampling, fp32 blending, nothing fused."""
    out = image.copy()
    for layer in layers:
        panel = panels[int(layer[0])]
        px0, py0, pw, ph = (int(v) for v in panel[:4])
        k = int(layer[8])
        rgb, alpha = [F32(v) for v in layer[17:20]], F32(layer[20])
        band, _ = bands_of(panel, layer, grids)
        view = out[:, py0:py0 + ph, px0:px0 + pw]
        if layer[21]:
            t = (np.minimum(band, k - 1).astype(F32) / F32(k - 1)) if k > 1 else np.ones(band.shape, F32)
            for q in range(3):
                shade = (F32(1) - t) + rgb[q] * t
                view[q] = np.where(band >= 1, view[q] * (F32(1) - alpha) + shade * alpha, view[q])
        if layer[22]:
            edge = np.zeros(band.shape, bool)
            edge[:, :-1] |= band[:, 1:] != band[:, :-1]
            edge[:-1, :] |= band[1:, :] != band[:-1, :]
            for q in range(3):
                view[q] = np.where(edge, view[q] * (F32(1) - alpha) + rgb[q] * alpha, view[q])
    return out


def layer_row(panel, offset, g, lo, step, levels, rgba, fill, line):
    row = np.zeros(ops.SHADE_LAYER_DOUBLES)
    row[:8] = [panel, offset, g[0], g[1], lo[0], step[0], lo[1], step[1]]
    row[8] = len(levels)
    row[9:9 + len(levels)] = levels
    row[17:21] = rgba
    row[21], row[22] = fill, line
    return row


def small_grids(seed, n=3, shape=(5, 5)):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 7, size=(n,) + shape).astype(np.float64)


THIRDS = [k + 1.0 / 3.0 for k in range(5)]


def run_shade(h, w, panels, layers, grids, seed=0):
    rng = np.random.default_rng(seed)
    image = rng.random((3, h, w)).astype(F32)
    flat = np.ascontiguousarray(grids.reshape(-1))
    got = ops.density_shade(torch.from_numpy(image).to(DEV), torch.from_numpy(flat).to(DEV), panels, layers)
    return image, got.cpu().numpy(), shade_reference(image, flat, np.asarray(panels, dtype=np.float64), layers)


def test_density_shade_two_panels_bit_for_bit():
    grids = small_grids(1)
    panels = [[0, 0, 64, 48, 0.0, 4.0, 0.5, 3.5],     # 16 pixels per cell on both axes
              [80, 8, 64, 48, 1.0, 3.0, 0.0, 3.0]]    # 32 and 16 pixels per cell, another window
    layers = [layer_row(0, 0, (5, 5), (0.0, 0.0), (1.0, 1.0), THIRDS, (0.9, 0.2, 0.1, 0.8), 1, 1),
              layer_row(1, 25, (5, 5), (0.0, 0.0), (1.0, 1.0), [2 + 1.0 / 3.0], (0.1, 0.3, 0.8, 1.0), 0, 1),
              # a support that covers only the middle of panel 1's window: [1.5, 2.5] x [1, 2]
              layer_row(1, 50, (5, 5), (1.5, 1.0), (0.25, 0.25), THIRDS[:3], (0.2, 0.7, 0.3, 0.5), 1, 0)]
    image, got, ref = run_shade(64, 160, panels, layers, grids)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    outside = np.ones((64, 160), bool)
    outside[0:48, 0:64] = False
    outside[8:56, 80:144] = False
    assert np.array_equal(got[:, outside].view(np.uint32), image[:, outside].view(np.uint32))
    assert (got != image).any(axis=0)[0:48, 0:64].mean() > 0.3 and (got != image)[:, 8:56, 80:144].any()
    # the partial layer paints nothing outside its support
    band, d = bands_of(panels[1], layers[2], grids.reshape(-1))
    assert (band > 0).any() and not d[:, :16].any() and not d[:, 48:].any()
    # every band of the five-level layer occurs
    assert set(np.unique(bands_of(panels[0], layers[0], grids.reshape(-1))[0])) >= {0, 1, 2, 3, 4, 5}


def test_density_shade_panel_cutting_tiles_bit_for_bit():
    grids = small_grids(2, n=2)
    panels = [[3, 5, 61, 43, 0.0, 4.0, 0.0, 4.0]]
    layers = [layer_row(0, 0, (5, 5), (0.0, 0.0), (1.0, 1.0), THIRDS, (0.1, 0.5, 0.9, 0.8), 1, 1),
              layer_row(0, 25, (5, 5), (0.0, 0.0), (1.0, 1.0), [1 + 1.0 / 3.0], (0.0, 0.0, 0.0, 0.5), 0, 1)]
    image, got, ref = run_shade(50, 70, panels, layers, grids, seed=3)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    outside = np.ones((50, 70), bool)
    outside[5:48, 3:64] = False
    assert np.array_equal(got[:, outside].view(np.uint32), image[:, outside].view(np.uint32))


def test_density_shade_more_layers_than_one_launch():
    """13 layers span two launches; the order of the blends is kept across them."""
    grids = small_grids(4, n=13)
    panels = [[0, 0, 64, 64, 0.0, 4.0, 0.0, 4.0]]
    layers = [layer_row(0, 25 * k, (5, 5), (0.0, 0.0), (1.0, 1.0), THIRDS[:1 + k % 5],
                        (0.07 * k, 1.0 - 0.07 * k, 0.5, 0.6), 1, k % 2) for k in range(13)]
    _, got, ref = run_shade(64, 64, panels, layers, grids, seed=5)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------- draw_primitives
def coverage_reference(q, fx, fy):
    """Coverage of pixel centres (fp32 arrays) by primitive row ``q``, in fp32."""
    kind, r = int(q[0]), F32(q[7])
    half, zero, one = F32(0.5), F32(0), F32(1)
    if kind == ops.PRIM_TRIANGLE:
        ax, ay, bx, by, cx, cy = (F32(v) for v in q[1:7])
        area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area2 == 0:
            return np.zeros(np.broadcast(fx, fy).shape, F32)
        s = F32(-1) if area2 > 0 else F32(1)

        def edge(px, py, qx, qy):
            return s * ((qx - px) * (fy - py) - (qy - py) * (fx - px)) / np.sqrt((qx - px) * (qx - px) + (qy - py) * (qy - py))

        e = np.maximum(edge(ax, ay, bx, by), np.maximum(edge(bx, by, cx, cy), edge(cx, cy, ax, ay)))
        return np.clip(half - e, zero, one).astype(F32)
    dx, dy = fx - F32(q[1]), fy - F32(q[2])
    if kind == ops.PRIM_SEGMENT:
        bx, by = F32(q[3]) - F32(q[1]), F32(q[4]) - F32(q[2])
        len2 = bx * bx + by * by
        if len2 > 0:
            h = np.clip((dx * bx + dy * by) / len2, zero, one)
            dx, dy = dx - bx * h, dy - by * h
    return np.clip(r + half - np.sqrt(dx * dx + dy * dy), zero, one).astype(F32)


def draw_reference(images, prims, prim_ptr):
    out = images.copy()
    b, _, h, w = images.shape
    fx, fy = np.arange(w, dtype=F32)[None, :] + F32(0.5), np.arange(h, dtype=F32)[:, None] + F32(0.5)
    touched = np.zeros((b, h, w), np.int32)
    for i in range(b):
        for q in prims[prim_ptr[i]:prim_ptr[i + 1]]:
            clip = (fx >= q[12]) & (fx <= q[14]) & (fy >= q[13]) & (fy <= q[15])
            cov = np.where(clip, coverage_reference(q, fx, fy), F32(0)).astype(F32)
            wgt = F32(q[11]) * cov
            for ch in range(3):
                out[i, ch] = np.where(cov > 0, out[i, ch] * (F32(1) - wgt) + F32(q[8 + ch]) * wgt, out[i, ch])
            touched[i] += cov > 0
    return out, touched


def far_from_all(prims, h, w, margin=1e-3):
    """Pixels farther than r + 1/2 (+ margin) from every primitive, in float64."""
    fx, fy = np.arange(w)[None, :] + 0.5, np.arange(h)[:, None] + 0.5
    far = np.ones((h, w), bool)
    for q in prims.astype(np.float64):
        kind = int(q[0])
        if kind == ops.PRIM_TRIANGLE:
            a, b, c = q[1:3], q[3:5], q[5:7]
            area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            if area2 == 0:
                continue
            s = -1.0 if area2 > 0 else 1.0
            e = np.full((h, w), -np.inf)
            for p, r in ((a, b), (b, c), (c, a)):
                e = np.maximum(e, s * ((r[0] - p[0]) * (fy - p[1]) - (r[1] - p[1]) * (fx - p[0])) / np.hypot(*(r - p)))
            dist, reach = e, 0.5
        else:
            dx, dy = fx - q[1], fy - q[2]
            bx, by = (q[3] - q[1], q[4] - q[2]) if kind == ops.PRIM_SEGMENT else (0.0, 0.0)
            if bx * bx + by * by > 0:
                t = np.clip((dx * bx + dy * by) / (bx * bx + by * by), 0, 1)
                dx, dy = dx - bx * t, dy - by * t
            dist, reach = np.hypot(dx, dy), q[7] + 0.5
        inside_clip = (fx >= q[12]) & (fx <= q[14]) & (fy >= q[13]) & (fy <= q[15])
        far &= ~inside_clip | (dist > reach + margin)
    return far


def prim(kind, geom, r, rgba, clip=(0, 0, 96, 80)):
    row = np.zeros(ops.PRIM_FLOATS, F32)
    row[0] = kind
    row[1:1 + len(geom)] = geom
    row[7] = r
    row[8:12] = rgba
    row[12:16] = clip
    assert np.array_equal(row[1:8] * 8, np.round(row[1:8] * 8))  # multiples of 1/8 pixel
    return row


def check_draw(images, prims, prim_ptr, what):
    got = ops.draw_primitives(torch.from_numpy(images).to(DEV), prims, prim_ptr).cpu().numpy()
    ref, touched = draw_reference(images, prims, prim_ptr)
    err = np.abs(got - ref).max()
    print(f"{what}: largest difference {err:.3e} (bound 1e-4), at most {touched.max()} primitives on a pixel")
    assert touched.max() <= 8 and err <= 1e-4, what
    for i in range(len(images)):
        far = far_from_all(prims[prim_ptr[i]:prim_ptr[i + 1]], *images.shape[2:])
        assert np.array_equal(got[i][:, far].view(np.uint32), images[i][:, far].view(np.uint32)), (what, i)
    return got, ref, touched


def test_draw_primitives_rounds_tiles_and_edge_cases():
    h, w, n = 80, 96, ops.PRIM_ROUND + 5
    rng = np.random.default_rng(0)
    images = rng.random((3, 3, h, w)).astype(F32)
    many = []
    for k in range(n):  # small discs on a 5-pixel lattice: none overlaps another
        cx, cy = 3.0 + 5 * (k % 19), 3.0 + 5 * (k // 19)
        many.append(prim(ops.PRIM_DISC, [cx + (k % 3) / 8.0, cy + (k % 5) / 8.0], 1.5,
                         (rng.random(), rng.random(), rng.random(), 0.25 + 0.75 * rng.random())))
    many[7] = prim(ops.PRIM_DISC, [32.0, 8.0], 3.0, (1, 0, 0, 0.7))                       # across a tile corner
    many[20] = prim(ops.PRIM_DISC, [60.5, 40.25], 6.0, (0, 1, 0, 0.9), clip=(58, 36, 64, 41))  # clipped
    many[33] = prim(ops.PRIM_DISC, [-20.0, -20.0], 4.0, (0, 0, 1, 1.0))                   # wholly off the image
    many[40] = prim(ops.PRIM_DISC, [120.0, 90.0], 10.0, (0, 0, 1, 1.0))                   # off the other corner
    many[50] = prim(ops.PRIM_TRIANGLE, [10.0, 60.0, 20.0, 65.0, 30.0, 70.0], 0.0, (1, 1, 0, 1.0))  # zero area
    many[60] = prim(ops.PRIM_SEGMENT, [70.5, 20.5, 70.5, 20.5], 2.5, (1, 0, 1, 0.8))      # zero length: a disc
    many[70] = prim(ops.PRIM_TRIANGLE, [40.0, 50.0, 58.5, 54.25, 45.0, 66.0], 0.0, (0, 1, 1, 0.6))
    many[71] = prim(ops.PRIM_TRIANGLE, [40.0, 50.0, 45.0, 66.0, 58.5, 54.25], 0.0, (1, 0.5, 0, 0.5))  # the other orientation
    many[80] = prim(ops.PRIM_SEGMENT, [5.0, 75.0, 90.0, 30.5], 0.75, (0.2, 0.2, 0.2, 0.9))
    many[n - 3] = prim(ops.PRIM_DISC, [18.0, 8.0], 7.5, (0.5, 0.0, 0.5, 0.5))              # second round, over round-one discs
    many[n - 1] = prim(ops.PRIM_SEGMENT, [0.0, 0.0, 95.0, 79.0], 0.5, (0, 0, 0, 1.0))      # second round, across every tile row
    one = [prim(ops.PRIM_DISC, [95.5, 79.5], 4.0, (1, 1, 1, 1.0))]                         # on the image's far corner
    prims = np.stack(one + many)
    got, ref, touched = check_draw(images, prims, [0, 0, 1, 1 + n], "0 / 1 / PRIM_ROUND + 5 primitives")
    assert np.array_equal(got[0].view(np.uint32), images[0].view(np.uint32))  # no primitive: untouched
    assert (got[1] != images[1]).any() and touched[2].max() >= 3
    # the zero-length segment is the disc of its half-width
    disc_img = ops.draw_primitives(torch.from_numpy(images[:1]).to(DEV),
                                   [prim(ops.PRIM_DISC, [70.5, 20.5], 2.5, (1, 0, 1, 0.8))], [0, 1]).cpu().numpy()
    seg_img = ops.draw_primitives(torch.from_numpy(images[:1]).to(DEV), [many[60]], [0, 1]).cpu().numpy()
    assert np.array_equal(disc_img, seg_img) and (disc_img != images[:1]).any()
    # the clipped disc changes nothing outside its rectangle, the off-image ones nothing at all
    only = ops.draw_primitives(torch.from_numpy(images[:1]).to(DEV), np.stack([many[20], many[33], many[40], many[50]]),
                               [0, 4]).cpu().numpy()
    changed = (only[0] != images[0]).any(axis=0)
    assert changed[36:41, 58:64].all() and changed.sum() == 30
    again = ops.draw_primitives(torch.from_numpy(images).to(DEV), prims, [0, 0, 1, 1 + n]).cpu().numpy()
    assert np.array_equal(got, again)  # two calls, equal bits


def test_draw_primitives_blends_in_order():
    rng = np.random.default_rng(1)
    images = rng.random((2, 3, 80, 96)).astype(F32)
    a = prim(ops.PRIM_DISC, [40.0, 40.0], 10.0, (1, 0, 0, 0.6))
    b = prim(ops.PRIM_DISC, [48.0, 44.0], 10.0, (0, 0, 1, 0.6))
    images[1] = images[0]
    got, ref, _ = check_draw(images, np.stack([a, b, b, a]), [0, 2, 4], "two discs in both orders")
    assert np.abs(got[0] - got[1]).max() > 0.1  # the order shows where they overlap
    assert np.abs(got[0] - got[1])[:, :30, :].max() == 0


def test_draw_primitives_acute_tips_across_tile_borders():
    """A tip of interior angle t is covered up to 1 / (2 sin(t / 2)) past its
    vertex (the mitre of the edge lines moved out by 1/2), not 1/2: tips of 11
    to 24 degrees lying 1/2 to 1 pixel inside a border of the 32 x 8 tiles and
    pointing across it, in all four directions, and the head of
    ``figures.arrow`` in the same place."""
    rng = np.random.default_rng(2)
    images = rng.random((2, 3, 80, 96)).astype(F32)
    images[1] = images[0]
    rgba = (0.1, 0.2, 0.9, 1.0)
    tips = [prim(ops.PRIM_TRIANGLE, [31.0, 20.5, 11.0, 18.5, 11.0, 22.5], 0.0, rgba),      # +x, across x = 32
            prim(ops.PRIM_TRIANGLE, [64.75, 60.5, 84.0, 58.5, 84.0, 62.5], 0.0, rgba),     # -x, across x = 64
            prim(ops.PRIM_TRIANGLE, [50.5, 39.25, 47.5, 25.0, 53.5, 25.0], 0.0, rgba),     # +y, across y = 40
            prim(ops.PRIM_TRIANGLE, [20.5, 48.5, 18.0, 64.0, 23.0, 64.0], 0.0, rgba),      # -y, across y = 48
            prim(ops.PRIM_TRIANGLE, [63.5, 8.5, 70.0, 0.5, 71.0, 2.0], 0.0, rgba)]         # towards a tile corner
    head = [q for q in figures.arrow((70.0, 30.5), (95.375, 30.5), "#a34D7a", (0, 0, 96, 80))
            if q[0] == ops.PRIM_TRIANGLE]                                                   # tip 5/8 inside x = 96
    head += [q for q in figures.arrow((12.0, 70.5), (31.25, 71.25), "#a34D7a", (0, 0, 96, 80)) if q[0] == ops.PRIM_TRIANGLE]
    prims = np.stack(tips + head)
    got, ref, _ = check_draw(images, np.concatenate([prims, prims[::-1]]), [0, len(prims), 2 * len(prims)],
                             "acute tips across tile borders")
    fx, fy = np.arange(96, dtype=F32)[None, :] + F32(0.5), np.arange(80, dtype=F32)[:, None] + F32(0.5)
    for q, (x, y) in zip(tips, [(32, 20), (63, 60), (50, 40), (20, 47)]):  # the pixel past the border is covered
        cov = coverage_reference(q, fx, fy)[y, x]
        assert cov > 0.2 and (got[0][:, y, x] != images[0][:, y, x]).any(), (x, y, cov)


def test_figures_wrappers_refuse_bad_arguments():
    points = torch.zeros(5, 2, dtype=torch.float64, device=DEV)
    row = [1, 0, 1, 1, 0, 0.1, 0, 0.1]
    for bad in (dict(points=points.float()), dict(points=points.cpu()), dict(points=points[:, :1]),
                dict(set_ptr=[0, 6]), dict(set_ptr=[0, 3, 2]), dict(set_ptr=[0]), dict(params=[row, row]),
                dict(params=[row[:7]]), dict(grid_size=1), dict(params=[[1, 0, 1, 1, 0, 0.0, 0, 0.1]])):
        args = {"points": points, "set_ptr": [0, 5], "params": [row], "grid_size": 9, **bad}
        with pytest.raises(ValueError):
            ops.kde2d(**args)
    image = torch.zeros(3, 48, 64, device=DEV)
    grids = torch.zeros(25, dtype=torch.float64, device=DEV)
    panel = [0, 0, 64, 48, 0.0, 4.0, 0.0, 4.0]
    layer = layer_row(0, 0, (5, 5), (0.0, 0.0), (1.0, 1.0), [0.5], (1, 0, 0, 1), 1, 0)
    nine = layer_row(0, 0, (5, 5), (0.0, 0.0), (1.0, 1.0), [0.5], (1, 0, 0, 1), 1, 0)
    nine[8] = 9
    for bad in (dict(image=image[0]), dict(image=image.double()), dict(grids=grids.float()), dict(grids=grids.cpu()),
                dict(panels=[panel] * 17), dict(panels=[panel[:7]]), dict(layers=[nine]), dict(layers=[layer[:20]])):
        args = {"image": image, "grids": grids, "panels": [panel], "layers": [layer], **bad}
        with pytest.raises(ValueError):
            ops.density_shade(**args)
    images = torch.zeros(2, 3, 80, 96, device=DEV)
    good = prim(ops.PRIM_DISC, [10.0, 10.0], 3.0, (1, 0, 0, 1))
    for bad in (dict(images=images[0]), dict(images=images.cpu()), dict(prim_ptr=[0, 1]), dict(prim_ptr=[0, 2, 1]),
                dict(prims=[prim(ops.PRIM_DISC, [10.0, 10.0], 3.0, (1, 0, 0, 1), clip=(0, 0, 97, 80))])):
        args = {"images": images, "prims": [good], "prim_ptr": [0, 1, 1], **bad}
        with pytest.raises(ValueError):
            ops.draw_primitives(**args)


# ---------------------------------------------------------------- end to end
TO_MM = 89.11
CONFIG = {
    "optimization": {"epochs": 2, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
    "classifier": {"main_model_type": "qda", "mlp_training_type": "after", "mlp_hidden_features": [32, 16],
                   "mlp_lr": 1e-3, "mlp_epochs": 2},
    "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
}
N_MESHES = 40
N_TRAIN = 32


@pytest.fixture(scope="module")
def planner(tmp_path_factory, topo_npz):
    """The recipe of ``test_gpu_planning.py``: a manager over the golden weights
    whose QDA, LDA and region classifiers are fitted on 40 encoded demo meshes
    (the 12 golden ones plus jittered copies, 10 per class n / a / c / m), three
    made-up procedures and a Tester; then the embedding figures drawn from the
    manager's own projections (the first 32 rows the training set, every fifth
    row marked augmented)."""
    from craniofacialsd_vae_amd import manager as M
    from craniofacialsd_vae_amd import precompute
    d = tmp_path_factory.mktemp("demo_figures")
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    (d / "meshes").mkdir()
    m = recipe.load_meshes()
    rs = np.random.RandomState(3)
    names, verts = [], []
    for i in range(N_MESHES):
        v = (m["verts"][i % 12] + (0 if i < 12 else rs.normal(0, 0.002, m["verts"][0].shape))).astype(np.float32)
        names.append(f"{'nacm'[i % 4]}_{i:03d}.obj")
        verts.append(v)
        with open(d / "meshes" / names[-1], "w") as f:
            for p in v:
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": TO_MM,
                             "swap_features": True, "stratified_split": False})
    man = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"], use_graph=False)
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    norm = {"mean": torch.from_numpy(m["norm_mean"]).float().contiguous(),
            "std": torch.from_numpy(m["norm_std"]).float().contiguous()}
    x = (torch.from_numpy(np.stack(verts)) - norm["mean"]) / norm["std"]
    z = man.encode(x.to(DEV).contiguous()).contiguous()
    letters = [n[0] for n in names]
    y = torch.tensor(man.class2idx(letters), dtype=torch.int32)
    man.lda.fit(z, y, n_classes=4)
    man.qda.fit(z, y, n_classes=4)
    for key, (lo, hi) in man.latent_regions.items():
        man.region_ldas[key].fit(z, y, cols=(lo, hi - lo), n_classes=4)
        man.region_qdas[key].fit(z, y, cols=(lo, hi - lo), n_classes=4)
    keys = [str(k) for k in man.latent_regions]
    cfg["planning"] = {"procedures": {"front": [keys[0], keys[1]], "middle": [keys[1], keys[5], keys[6]],
                                      "last": [keys[14]]}}
    stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
    tester = evaluation.Tester(man, norm, None, None, str(d / "out"), cfg, latent_stats=stats, animations=True)
    xy = man.lda_project_latents_in_2d(z)
    xy = torch.stack([xy[:, 0], xy[:, -1]], dim=1).cpu().numpy()
    is_test = np.arange(N_MESHES) >= N_TRAIN
    augmented = np.arange(N_MESHES) % 5 == 4
    regions = {k: np.asarray(v) for k, v in tester._region_projections(z[:N_TRAIN]).items()}
    out = figures.embedding_figures(xy, np.array(letters), is_test, augmented, str(d / "out"), prefix="lda",
                                    regions=regions, device=DEV)
    tester.figure_bases = {"lda": out}
    return {"dir": d, "manager": man, "tester": tester, "names": names, "z": z, "keys": keys, "figures": out,
            "heads": x.to(DEV).contiguous(), "norm": norm, "cfg": cfg,
            "xy": xy, "letters": np.array(letters), "is_test": is_test, "augmented": augmented, "regions": regions}


def png(path):
    w, h, rgb = decode_png(str(path))
    return (w, h), rgb


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_embedding_figures_end_to_end(planner):
    out, d = planner["figures"], planner["dir"] / "out"
    names = {"train_vs_test": "lda_emb_train_vs_test.png", "real_vs_aug": "lda_emb_real_vs_aug.png",
             "real_dist_vs_sc_aug": "lda_emb_real_dist_vs_sc_aug.png", "distributions": "lda_emb_distributions.png",
             "all_train": "emb_all_train.png", "all_train_dist": "emb_all_train_dist.png"}
    assert set(out) == set(names)
    for key, name in names.items():
        size, rgb = png(d / name)
        assert size == ((640, 480) if name.startswith("lda_") else (1000, 600)), name
        assert out[key]["path"] == str(d / name) and tuple(out[key]["image"].shape) == (3, size[1], size[0])
        assert np.array_equal(rgb, ((out[key]["image"].clamp(0, 1) * 255 + 0.5).floor().byte().permute(1, 2, 0)
                                    .cpu().numpy())), name
        assert (rgb != 255).any(), name
    side = json.load(open(d / "figures.json"))
    assert set(side) == set(names.values())
    npz = np.load(d / "lda_emb_density.npz")
    density, share, group, cls = npz["density"], npz["share"], npz["group"], npz["class"]
    assert density.shape == (len(cls), 200, 200) and npz["support"].shape == (len(cls), 2, 200)
    main = [s for s in range(len(cls)) if group[s] == "main"]
    assert [cls[s] for s in main] == ["n", "a", "c", "m"] and side["lda_emb_distributions.png"]["skipped"] == {"lda": {}}
    # the saved grids are what scipy gives for the real training rows
    real = ~planner["is_test"] & ~planner["augmented"]
    for s in main:
        pts = planner["xy"][real & (planner["letters"] == cls[s])]
        assert len(pts) == npz["set_ptr"][s + 1] - npz["set_ptr"][s]
        check_density(density[s], kde_reference(pts, npz["params"][s], 200), f"class {cls[s]}")
        assert share[s] == len(pts) / real.sum()
    # the levels of the sidecar are the host rule on the saved grids
    q5, q68 = np.linspace(0.05, 1, 5), [0.68]
    for s in main:
        assert side["lda_emb_distributions.png"]["levels"]["lda"][cls[s]] == figures.iso_levels(density[s], q5).tolist()
    common = figures.iso_levels([density[s] * share[s] for s in main], q5).tolist()
    assert all(v == common for v in side["lda_emb_real_dist_vs_sc_aug.png"]["levels"]["lda"].values())
    for r, key in enumerate(planner["keys"]):
        sets = [s for s in range(len(cls)) if group[s] == key]
        want = figures.iso_levels([density[s] * share[s] for s in sets], q68).tolist() if sets else None
        got = side["emb_all_train_dist.png"]["levels"][key]
        assert all(v == want for v in got.values()) and set(got) == {cls[s] for s in sets}, key
        panel = side["emb_all_train_dist.png"]["panels"][r]
        assert panel["name"] == key and panel["rect"] == [(r % 5) * 200 + 12, (r // 5) * 200 + 12, 176, 176]


@pytest.fixture(scope="module")
def distributions(planner):
    """``lda_emb_distributions.png`` with what it was drawn from: the decoded
    picture, the side file's entry, the panel and, per class, the band of every
    pixel centre of the panel under that class's levels (the restatement's
    sampling), the pixels that hold a node at or above its lowest level and the
    pixel that holds its highest node (both relative to the panel)."""
    d = planner["dir"] / "out"
    info = json.load(open(d / "figures.json"))["lda_emb_distributions.png"]
    npz = np.load(d / "lda_emb_density.npz")
    density, cls = npz["density"], npz["class"]
    main = [s for s in range(len(cls)) if npz["group"][s] == "main"]
    panel = info["panels"][0]
    px0, py0, pw, ph = panel["rect"]
    prow = np.array(panel["rect"] + panel["window"], dtype=np.float64)
    layers, bands, holds, peak = [], {}, {}, {}
    for s in main:
        c = str(cls[s])
        rgb = figures.rgb_of(info["colours"][c])
        for alpha, fill, line in ((0.8, 1, 0), (0.5, 0, 1)):
            layers.append(layer_row(0, s * 40000, (200, 200), npz["params"][s][[4, 6]], npz["params"][s][[5, 7]],
                                    info["levels"]["lda"][c], (*rgb, alpha), fill, line))
        bands[c] = bands_of(prow, layers[-1], density.reshape(-1))[0]
        gx, gy = np.meshgrid(npz["support"][s][0], npz["support"][s][1], indexing="ij")
        pix = np.floor(figures.to_pixels(panel, np.stack([gx.ravel(), gy.ravel()], axis=1))).astype(int) - [px0, py0]
        pix = np.clip(pix, 0, [pw - 1, ph - 1])
        inside = density[s].ravel() >= info["levels"]["lda"][c][0]
        holds[c] = np.zeros((ph, pw), bool)
        holds[c][pix[inside, 1], pix[inside, 0]] = True
        peak[c] = tuple(pix[int(np.argmax(density[s]))])
    replay = shade_reference(np.ones((3, 480, 640), F32), density.reshape(-1), prow[None], layers)
    for c, (x, y) in info["marked"]["lda"].items():  # the one-pixel marks, at alpha 0.8 over what was shaded
        replay[:, y, x] = replay[:, y, x] * F32(0.2) + np.array(figures.rgb_of(info["colours"][c]), F32) * F32(0.8)
    return {"rgb": png(d / "lda_emb_distributions.png")[1], "info": info, "panel": panel, "bands": bands,
            "holds": holds, "peak": peak, "replay": replay}


def interior(mask):
    """``mask`` without the two outermost pixels of the panel (its frame)."""
    mask = mask.copy()
    mask[:2], mask[-2:], mask[:, :2], mask[:, -2:] = False, False, False, False
    return mask


def top_band_alone(dist, c):
    """Pixels inside class ``c``'s top band -- those whose centre lies in it or,
    when the band holds no pixel centre, the pixel that holds the class's peak --
    that no other class reaches and no iso-line of ``c`` crosses."""
    bands, b = dist["bands"], dist["bands"][c]
    top = b >= 4
    if not top.any():
        top[dist["peak"][c][1], dist["peak"][c][0]] = True
    others = np.any([(o >= 1) | dist["holds"][k] for k, o in bands.items() if k != c], axis=0)
    alone = top & ~others
    alone[:, :-1] &= b[:, 1:] == b[:, :-1]
    alone[:-1, :] &= b[1:, :] == b[:-1, :]
    return interior(alone)


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_distributions_figure_replayed(distributions):
    """The picture equals the restatement replayed on the run's own layout,
    layers, grids and marks; outside every class's lowest level -- pixels that
    neither lie in it by their centre, nor hold a node of it, nor neighbour
    one that does -- the panel is white."""
    rgb, panel, bands = distributions["rgb"], distributions["panel"], distributions["bands"]
    px0, py0, pw, ph = panel["rect"]
    inner = (slice(py0 + 2, py0 + ph - 2), slice(px0 + 2, px0 + pw - 2))  # off the frame
    want = np.floor(np.clip(distributions["replay"], 0, 1) * 255 + 0.5).astype(np.int64).transpose(1, 2, 0)[inner]
    assert np.abs(rgb[inner].astype(np.int64) - want).max() <= 1  # (a blend on a rounding boundary may fall either way)
    view = rgb[py0:py0 + ph, px0:px0 + pw]
    any_band = np.zeros((ph, pw), bool)
    for c, b in bands.items():
        any_band |= (b >= 1) | distributions["holds"][c]
    blank = ~any_band
    blank[:, :-1] &= ~any_band[:, 1:]
    blank[:-1, :] &= ~any_band[1:, :]
    blank = interior(blank)
    assert blank.any() and (view[blank] == 255).all()


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_distributions_figure_shows_every_class(planner, distributions):
    """Every class's colour appears inside its top band: the band has at least
    one pixel that no other class reaches, and every such pixel shows the
    class's colour at alpha 0.8 on white.

    On this recipe the main LDA is fitted on 40 latents of 75 variables, so the
    fitted rows of a class collapse onto one point of the projection (kernel
    standard deviations of about 0.01 in a data window of 2260 x 1310, 1 / 400
    of a pixel): no pixel centre lies inside any class's lowest level, the
    shading kernel draws nothing of it, and the class shows by the one pixel
    that holds its peak (``figures.unseen_peak``, listed under ``marked``)."""
    bands, panel, info = distributions["bands"], distributions["panel"], distributions["info"]
    px0, py0, pw, ph = panel["rect"]
    view = distributions["rgb"][py0:py0 + ph, px0:px0 + pw]
    real = ~planner["is_test"] & ~planner["augmented"]
    lone = {}
    for c, b in bands.items():
        sd = np.sqrt(np.diag(figures.kde_covariance(planner["xy"][real & (planner["letters"] == c)])))
        alone = top_band_alone(distributions, c)
        lone[c] = int(alone.sum())
        print(f"class {c}: {int((b >= 1).sum())} pixel centres inside its lowest level, {int((b >= 4).sum())} in its top "
              f"band, {lone[c]} pixels of the band alone; kernel sd {sd[0]:.3g} x {sd[1]:.3g} in a window of "
              f"{panel['window'][1] - panel['window'][0]:.3g} x {panel['window'][3] - panel['window'][2]:.3g}")
        pure = np.floor((0.2 + 0.8 * np.array(figures.rgb_of(info["colours"][c]))) * 255 + 0.5)
        assert alone.any() and np.abs(view[alone].astype(np.float64) - pure).max() <= 1, c
        # a class is marked exactly when no pixel centre lies in its top band, and then at its peak's pixel
        x, y = distributions["peak"][c]
        assert info["marked"]["lda"].get(c) == (None if (b >= 4).any() else [px0 + int(x), py0 + int(y)]), c


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_region_sheet_replayed(planner):
    """Every panel of ``emb_all_train_dist.png`` equals the restatement replayed
    on the common-norm grids (each saved grid times its class's share), the
    side file's levels and marks: the layers the composition hands
    ``density_shade`` for a sheet of panels, their grid offsets included.  The
    region LDAs are fitted on 40 rows of 5 variables, so their classes span
    pixels and the 0.68 lines are really drawn."""
    d = planner["dir"] / "out"
    info = json.load(open(d / "figures.json"))["emb_all_train_dist.png"]
    npz = np.load(d / "lda_emb_density.npz")
    density, share, cls, group = npz["density"], npz["share"], npz["class"], npz["group"]
    common = density * share[:, None, None]
    _, rgb = png(d / "emb_all_train_dist.png")
    drawn = 0
    for r, panel in enumerate(info["panels"]):
        sets = [s for s in range(len(cls)) if group[s] == panel["name"]]
        prow = np.array(panel["rect"] + panel["window"], dtype=np.float64)
        layers = [layer_row(0, s * 40000, (200, 200), npz["params"][s][[4, 6]], npz["params"][s][[5, 7]],
                            info["levels"][panel["name"]][str(cls[s])],
                            (*figures.rgb_of(info["colours"][str(cls[s])]), 1.0), 0, 1) for s in sets]
        replay = shade_reference(np.ones((3, 600, 1000), F32), common.reshape(-1), prow[None], layers)
        for c, (x, y) in info["marked"][panel["name"]].items():
            replay[:, y, x] = np.array(figures.rgb_of(info["colours"][c]), F32)
        px0, py0, pw, ph = panel["rect"]
        inner = (slice(py0 + 2, py0 + ph - 2), slice(px0 + 2, px0 + pw - 2))  # off the frame
        want = np.floor(np.clip(replay, 0, 1) * 255 + 0.5).astype(np.int64).transpose(1, 2, 0)[inner]
        assert np.abs(rgb[inner].astype(np.int64) - want).max() <= 1, panel["name"]
        lines = int((want != 255).any(axis=-1).sum()) - len(info["marked"][panel["name"]])
        drawn += lines > 50
        # the legend strip of the panel, in the margin above it: one swatch per class, in the class colours
        for k, c in enumerate("nacm"):
            swatch = rgb[py0 - 6, px0 + 3 + 14 * k + 4].astype(np.float64)
            assert np.abs(swatch - np.floor(np.array(figures.rgb_of(info["colours"][c])) * 255 + 0.5)).max() <= 1, (r, c)
    print(f"{drawn} of {len(info['panels'])} region panels have iso-lines of more than 50 pixels")
    assert drawn >= 1  # (the replay above is of drawn lines, not of blank panels)


def sets_tester(planner, out_dir):
    """A second Tester on the planner's manager, with the 40 heads as train (32) and test (8) sets."""
    import types
    t0, z = planner["tester"], planner["z"]
    heads = planner["heads"]
    labels = [(str(c), bool(a)) for c, a in zip(planner["letters"], planner["augmented"])]
    sets = [types.SimpleNamespace(meshes=heads[s].contiguous(), labels=labels[s])
            for s in (slice(0, N_TRAIN), slice(N_TRAIN, N_MESHES))]
    stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
    return evaluation.Tester(planner["manager"], planner["norm"], sets[0], sets[1], str(out_dir), planner["cfg"],
                             latent_stats=stats, animations=False)


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_step_figures_through_the_tester(planner, tmp_path):
    """``Tester.run("figures")`` with a patient and a pairs table: the arrays of
    ``embeddings()`` reach ``figures.embedding_figures`` (the same rows, classes
    and flags as the planner's direct call), the plan and pair figures are
    written; then the t-SNE mode on the same folder: prefix ``tsne``, no region
    sheet, and ``figures.json`` keeps the entries of both prefixes."""
    d, names = planner["dir"], planner["names"]
    t = sets_tester(planner, tmp_path / "out")
    pairs_csv = tmp_path / "pairs.csv"
    rows = [("p1", names[1], names[4], "front", "monobloc", "Apert"), ("p2", names[2], names[8], "last", "lefort", "Crouzon")]
    with open(pairs_csv, "w") as f:
        f.write(",".join(evaluation.PAIR_COLUMNS) + "\n" + "".join(",".join(r) + "\n" for r in rows))
    t.plan_patients, t.pairs_table, t.pairs_root = (str(d / "meshes" / names[1]),), str(pairs_csv), str(d / "meshes")
    out = t.run("figures")
    assert set(out) == {"lda", "plan", "prepost"} and t.figure_bases["lda"] is out["lda"]
    root = tmp_path / "out"
    lda_files = ["lda_emb_train_vs_test.png", "lda_emb_real_vs_aug.png", "lda_emb_real_dist_vs_sc_aug.png",
                 "lda_emb_distributions.png", "emb_all_train.png", "emb_all_train_dist.png"]
    side = json.load(open(root / "figures.json"))
    assert sorted(side) == sorted(lda_files) and all((root / f).exists() for f in lda_files)
    assert (root / "lda_embeddings.npz").exists()
    npz, ref = np.load(root / "lda_emb_density.npz"), np.load(d / "out" / "lda_emb_density.npz")
    assert npz["class"].tolist() == ref["class"].tolist() and npz["group"].tolist() == ref["group"].tolist()
    assert npz["set_ptr"].tolist() == ref["set_ptr"].tolist() and np.array_equal(npz["share"], ref["share"])
    assert np.allclose(npz["params"], ref["params"], rtol=1e-3)  # (the same rows, projected in two batches)
    assert [p["name"] for p in side["emb_all_train_dist.png"]["panels"]] == planner["keys"]
    assert list(out["plan"][0]) == ["all_attributes", "front", "middle", "last"]
    for name, files in out["plan"][0].items():
        assert sorted(files) == ["emb", "emb_r"] and all(os.path.exists(p) for p in files.values()), name
    assert sorted(os.listdir(root / "pre_post_eval_plots")) == ["p1_emb.png", "p1_emb_r.png", "p2_emb.png",
                                                                 "p2_emb_r.png"]
    # the t-SNE mode, fitted here since no tsne_embeddings.npz exists yet
    more = t.embedding_figures("tsne")
    tsne_files = [f.replace("lda_", "tsne_") for f in lda_files[:4]]
    assert sorted(more) == ["distributions", "real_dist_vs_sc_aug", "real_vs_aug", "train_vs_test"]
    assert (root / "tsne_embeddings.npz").exists() and all(png(root / f)[0] == (640, 480) for f in tsne_files)
    side = json.load(open(root / "figures.json"))
    assert sorted(side) == sorted(lda_files + tsne_files) and set(t.figure_bases) == {"lda", "tsne"}
    emb, dens = np.load(root / "tsne_embeddings.npz"), np.load(root / "tsne_emb_density.npz")
    assert set(dens["group"].tolist()) == {"main"} and dens["density"].shape[1:] == (200, 200)
    real = ~emb["is_test"] & ~emb["augmented"]
    assert dens["set_ptr"][-1] == real.sum() and emb["class"].tolist() == planner["letters"].tolist()
    with pytest.raises(NotImplementedError):
        t.embedding_figures("pca")


def test_evaluate_only_figures(planner, tmp_path):
    """One epoch without a classifier section, then ``evaluate.py --only
    figures``: on a run that has no classifier files the step draws the t-SNE
    figures, and nothing else."""
    import yaml

    from craniofacialsd_vae_amd import train as T
    cfg = {k: v for k, v in planner["cfg"].items() if k not in ("classifier", "planning")}
    cfg["optimization"] = dict(cfg["optimization"], epochs=1)
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    T.main(["--config", str(tmp_path / "config.yaml"), "--id", "fg", "--output_path", str(tmp_path / "runs")])
    tester = evaluation.evaluate_main(["--id", "fg", "--output_path", str(tmp_path / "runs"), "--seed", "5",
                                       "--only", "figures"])
    assert not tester.has_classifiers and set(tester.figure_bases) == {"tsne"}
    root = tmp_path / "runs" / "outputs" / "fg"
    files = ["tsne_emb_train_vs_test.png", "tsne_emb_real_vs_aug.png", "tsne_emb_real_dist_vs_sc_aug.png",
             "tsne_emb_distributions.png"]
    assert sorted(json.load(open(root / "figures.json"))) == sorted(files)
    assert all(png(root / f)[0] == (640, 480) for f in files) and not (root / "emb_all_train.png").exists()
    n_all = tester._train_set.meshes.shape[0] + tester._test_set.meshes.shape[0]
    assert np.load(root / "tsne_embeddings.npz")["x1"].shape == (n_all,)


def differs_only_near(frame, base, centres, radius, what):
    """``frame`` equals ``base`` except within ``radius`` of one of ``centres`` (pixels)."""
    changed = (frame != base).any(axis=-1)
    ys, xs = np.nonzero(changed)
    if not len(centres):
        assert not len(ys), what
        return 0
    c = np.asarray(centres, dtype=np.float64)
    dist = np.hypot(xs[:, None] + 0.5 - c[None, :, 0], ys[:, None] + 0.5 - c[None, :, 1]).min(axis=1)
    assert not len(ys) or dist.max() <= radius, (what, float(dist.max()))
    return len(ys)


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_plan_figures_end_to_end(planner):
    t, man, d = planner["tester"], planner["manager"], planner["dir"]
    patient = d / "meshes" / planner["names"][1]  # an 'a'
    files = t.plan_figures(str(patient))
    groups, f = ["all_attributes", "front", "middle", "last"], evaluation.PLAN_FIRST + 3
    assert list(files) == groups
    plan = t.plan_to_normal(t._load_and_encode(str(patient)))
    reach = figures.PATH_RADIUS + 0.5 + 1e-6
    bases = {"emb": planner["figures"]["distributions"], "emb_r": planner["figures"]["all_train_dist"]}
    base_rgb = {tag: (b["image"].clamp(0, 1) * 255 + 0.5).floor().byte().permute(1, 2, 0).cpu().numpy()
                for tag, b in bases.items()}
    for g, name in enumerate(groups):
        sub = d / "out" / "interpolations" / f"a_001_{name}"
        z = plan["tables"][0, g]
        xy = man.lda_project_latents_in_2d(z)
        centres = {"emb": [figures.to_pixels(bases["emb"]["layout"]["panels"][0], [[float(p[0]), float(p[-1])]])
                           for p in xy.cpu()]}
        region_xy = t._region_projections(z)
        centres["emb_r"] = [np.concatenate([figures.to_pixels(bases["emb_r"]["layout"]["panels"][k], [v[i]])
                                            for k, v in enumerate(region_xy.values())]) for i in range(f)]
        for tag in ("emb", "emb_r"):
            assert files[name][tag] == str(sub / f"a_001_{name}_{tag}_interpolate.png")
            size, whole = png(files[name][tag])
            assert (size[1], size[0]) == tuple(bases[tag]["layout"]["size"])
            every = np.concatenate([np.asarray(c).reshape(-1, 2) for c in centres[tag]])
            assert differs_only_near(whole, base_rgb[tag], every, reach, (name, tag)) > 0
            shots = check_apng(files[name][tag + "_animation"], f, fps=4)  # as many frames as the path has points
            assert shots.shape[1:] == base_rgb[tag].shape
            drawn = [differs_only_near(shots[i], base_rgb[tag], np.asarray(centres[tag][i]).reshape(-1, 2), reach,
                                       (name, tag, i)) for i in range(f)]
            assert max(drawn) > 0, (name, tag)
    # a frame's marker sits on its point: the first frame of the first group is the patient
    shots = check_apng(files["all_attributes"]["emb_animation"], f, fps=4)
    p = figures.to_pixels(bases["emb"]["layout"]["panels"][0],
                          [[float(v) for v in man.lda_project_latents_in_2d(plan["tables"][0, 0, :1])[0, [0, -1]].cpu()]])[0]
    px0, py0, pw, ph = bases["emb"]["layout"]["panels"][0]["rect"]
    if px0 + 1 <= p[0] < px0 + pw - 1 and py0 + 1 <= p[1] < py0 + ph - 1:
        want = np.floor(np.array(figures.rgb_of(figures.PATH_COLOUR)) * 255 + 0.5)
        assert np.abs(shots[0][int(p[1]), int(p[0])].astype(np.float64) - want).max() <= 1


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_prepost_figures_end_to_end(planner):
    t, d, z = planner["tester"], planner["dir"], planner["z"]
    ids = ["p1", "p2", "p3"]
    files = t.prepost_figures(z[[1, 2, 13]], z[[4, 8, 13]], ids)  # the last pair has not moved: points, no arrow
    assert list(files) == ids
    bases = {"emb": planner["figures"]["distributions"], "emb_r": planner["figures"]["all_train_dist"]}
    for pid in ids:
        for tag in ("emb", "emb_r"):
            assert files[pid][tag] == str(d / "out" / "pre_post_eval_plots" / f"{pid}_{tag}.png")
            size, rgb = png(files[pid][tag])
            assert (size[1], size[0]) == tuple(bases[tag]["layout"]["size"])
            base = (bases[tag]["image"].clamp(0, 1) * 255 + 0.5).floor().byte().permute(1, 2, 0).cpu().numpy()
            assert (rgb != base).any(), (pid, tag)
    assert sorted(os.listdir(d / "out" / "pre_post_eval_plots")) == sorted(f"{p}_{tag}.png" for p in ids
                                                                            for tag in ("emb", "emb_r"))
    with pytest.raises(ValueError, match="same pairs"):
        t.prepost_figures(z[:2], z[:3], ["a", "b"])
