"""``python tools/bench_figures.py [--out FILE]``: one set of embedding figures
on the GPU, one JSON line, printed and written to
``profiles/figures_bench.json`` (or ``FILE``; ``--out ''`` only prints).

The figure set of a 2 000-mesh training set: 64 kernel density estimates (the
4 classes of the main embedding and of 15 region embeddings, 900 / 420 / 380 /
300 rows) on 200 x 200 grids, the two density figures shaded from them, and 12
overlay frames.  Kernel figures are the median of ``--repeats`` (>= 5) timed
repeats after a warm-up, wall clock around work that ends in a device
synchronise, each alternating in the same run with the same arithmetic done
with torch operators on the same GPU.

* ``kde2d_ms``: ``ops.kde2d``, all 64 sets in one call.  ``torch_kde_ms``: per
  set the whitened differences of 10 000 nodes at a time against all points,
  ``exp`` and ``sum`` in float64.  ``kde_max_rel_diff``: the two compared.
* ``shade_ms``: ``ops.density_shade`` of the per-class figure (4 classes, filled
  bands and lines) and of the region sheet (15 panels, 60 line layers).
  ``torch_shade_ms``: the same sampling, bands and blends with torch indexing
  per layer.  ``shade_max_diff``: the two images compared.
* ``overlay_ms``: ``figures.overlay`` of 12 frames with one marker each on a 640
  x 480 figure (replication, table upload and one launch).
  ``torch_overlay_ms``: per frame the coverage of the whole image and the blend
  with torch operators.  ``overlay_max_diff``: the two compared.
* ``figure_set_s``: one whole ``figures.embedding_figures`` (densities, levels on
  the host, six figures, PNG and side files written).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CLASS_ROWS = {"n": 900, "a": 420, "c": 380, "m": 300}
REGIONS = 15
FRAMES = 12


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median_pair(a, b, repeats, warmup):
    """Medians (seconds) of ``a`` and ``b`` timed in alternating order."""
    for _ in range(warmup):
        a()
        b()
    ta, tb = [], []
    for r in range(repeats):
        for fn, out in ((a, ta), (b, tb)) if r % 2 == 0 else ((b, tb), (a, ta)):
            out.append(wall(fn))
    return statistics.median(ta), statistics.median(tb)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "figures_bench.json"),
                    help="file that receives the line ('' = none)")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import numpy as np
    import torch

    import cfsd_loader
    cfsd_loader.load()
    from craniofacialsd_vae_amd import figures, ops

    if not torch.cuda.is_available():
        raise RuntimeError("bench_figures measures on the GPU; no GPU visible")
    dev = torch.device("cuda", 0)
    G = figures.GRID
    res = {"bench": "figures", "device": torch.cuda.get_device_name(0), "repeats": opts.repeats,
           "sets": 4 * (1 + REGIONS), "grid": G, "rows": sum(CLASS_ROWS.values()), "frames": FRAMES}

    # ---- the seeded embeddings: four overlapping classes, in the main embedding and in every region
    rng = np.random.default_rng(0)
    classes = np.concatenate([[c] * n for c, n in CLASS_ROWS.items()])
    centres = {"n": (0.0, 0.0), "a": (2.5, 1.0), "c": (-1.5, 2.0), "m": (1.0, -2.5)}

    def embedding():
        mix = rng.standard_normal((2, 2)) * 0.4 + np.eye(2)
        return np.concatenate([rng.standard_normal((n, 2)) @ mix + centres[c] for c, n in CLASS_ROWS.items()])

    xy = embedding()
    regions = {f"r{r}": embedding() for r in range(REGIONS)}
    sets = [e[classes == c] for e in [xy] + list(regions.values()) for c in CLASS_ROWS]
    params = np.array([figures.kde_params(x) for x in sets])
    set_ptr = np.concatenate([[0], np.cumsum([len(x) for x in sets])])
    points = torch.from_numpy(np.concatenate(sets)).to(dev).contiguous()
    d_params = torch.from_numpy(params).to(dev)
    node = torch.arange(G, device=dev, dtype=torch.float64)

    def torch_kde():
        out = torch.empty((len(sets), G * G), dtype=torch.float64, device=dev)
        for s in range(len(sets)):
            p = d_params[s]
            x = points[set_ptr[s]:set_ptr[s + 1]]
            g = torch.stack(torch.meshgrid(p[4] + node * p[5], p[6] + node * p[7], indexing="ij"), dim=-1).view(-1, 2)
            for n0 in range(0, G * G, 10000):
                d = g[n0:n0 + 10000, None, :] - x[None]
                u0, u1 = p[0] * d[..., 0] + p[1] * d[..., 1], p[2] * d[..., 1]
                out[s, n0:n0 + 10000] = p[3] * torch.exp(-0.5 * (u0 * u0 + u1 * u1)).sum(1)
        return out.view(len(sets), G, G)

    a, b = median_pair(lambda: ops.kde2d(points, set_ptr, params, G), torch_kde, opts.repeats, opts.warmup)
    density, ref = ops.kde2d(points, set_ptr, params, G), torch_kde()
    res.update(kde2d_ms=a * 1e3, torch_kde_ms=b * 1e3,
               kde_max_rel_diff=float(((density - ref).abs() / ref.clamp_min(1e-300)).max()))

    # ---- the two density figures from those grids
    host = density.cpu().numpy()
    grids = density.reshape(-1).contiguous()
    colours = [figures.rgb_of(figures.CLASS_COLOURS[c]) for c in CLASS_ROWS]
    q5, q68 = figures.iso_proportions(5, 0.05), figures.iso_proportions(1, 0.68)
    main_panel = {"name": "main", "rect": list(figures.MAIN_PANEL),
                  "window": figures._window([xy] + [c for s in range(4) for c in figures._support_corners(params[s])])}
    main_layers = []
    for s in range(4):
        lv = figures.iso_levels(host[s], q5)
        main_layers.append(figures._layer(0, s * G * G, params[s], lv, figures.CLASS_COLOURS[classes[set_ptr[s]]],
                                          figures.DIST_FILL_ALPHA, True, False))
        main_layers.append(figures._layer(0, s * G * G, params[s], lv, figures.CLASS_COLOURS[classes[set_ptr[s]]],
                                          figures.DIST_LINE_ALPHA, False, True))
    side = figures.REGION_PANEL - 2 * figures.REGION_MARGIN
    region_panels, region_layers = [], []
    for r, e in enumerate(regions.values()):
        sl = range(4 + 4 * r, 8 + 4 * r)
        region_panels.append({"name": f"r{r}", "rect": [(r % 5) * 200 + 12, (r // 5) * 200 + 12, side, side],
                              "window": figures._window([e] + [c for s in sl for c in figures._support_corners(params[s])])})
        for k, s in enumerate(sl):
            region_layers.append(figures._layer(r, s * G * G, params[s], figures.iso_levels(host[s], q68),
                                                list(figures.CLASS_COLOURS.values())[k], 1.0, False, True))
    jobs = [((480, 640), [main_panel], main_layers), ((600, 1000), region_panels, region_layers)]

    def kernel_shade():
        return [ops.density_shade(torch.ones((3, *size), device=dev), grids, [figures._panel_row(p) for p in panels],
                                  layers) for size, panels, layers in jobs]

    def torch_shade():
        out = []
        for size, panels, layers in jobs:
            image = torch.ones((3, *size), device=dev)
            for L in layers:
                px0, py0, pw, ph = panels[int(L[0])]["rect"]
                xlo, xhi, ylo, yhi = panels[int(L[0])]["window"]
                x = torch.arange(px0, px0 + pw, device=dev, dtype=torch.float64)[None, :]
                y = torch.arange(py0, py0 + ph, device=dev, dtype=torch.float64)[:, None]
                u = ((xlo + (x + 0.5 - px0) / pw * (xhi - xlo)) - L[4]) / L[5] + 0 * y
                v = ((yhi - (y + 0.5 - py0) / ph * (yhi - ylo)) - L[6]) / L[7] + 0 * x
                inside = (u >= 0) & (u <= G - 1) & (v >= 0) & (v <= G - 1)
                i0 = torch.where(inside, u, torch.zeros_like(u)).long().clamp_max(G - 2)
                j0 = torch.where(inside, v, torch.zeros_like(v)).long().clamp_max(G - 2)
                fu, fv = u - i0, v - j0
                g = grids[int(L[1]):int(L[1]) + G * G].view(G, G)
                d = (g[i0, j0] * (1 - fu) + g[i0 + 1, j0] * fu) * (1 - fv) + \
                    (g[i0, j0 + 1] * (1 - fu) + g[i0 + 1, j0 + 1] * fu) * fv
                d = torch.where(inside, d, torch.zeros_like(d))
                k = int(L[8])
                band = (torch.tensor(L[9:9 + k], device=dev)[:, None, None] <= d[None]).sum(0)
                rgb = torch.tensor(L[17:20], device=dev, dtype=torch.float32)[:, None, None]
                alpha = float(L[20])
                view = image[:, py0:py0 + ph, px0:px0 + pw]
                if L[21]:
                    t = (band.clamp_max(k - 1).float() / (k - 1)) if k > 1 else torch.ones_like(band).float()
                    shade = (1 - t)[None] + rgb * t[None]
                    view.copy_(torch.where((band >= 1)[None], view * (1 - alpha) + shade * alpha, view))
                if L[22]:
                    edge = torch.zeros_like(band, dtype=torch.bool)
                    edge[:, :-1] |= band[:, 1:] != band[:, :-1]
                    edge[:-1, :] |= band[1:, :] != band[:-1, :]
                    view.copy_(torch.where(edge[None], view * (1 - alpha) + rgb * alpha, view))
            out.append(image)
        return out

    a, b = median_pair(kernel_shade, torch_shade, opts.repeats, opts.warmup)
    res.update(shade_layers=len(main_layers) + len(region_layers), shade_ms=a * 1e3, torch_shade_ms=b * 1e3,
               shade_max_diff=max(float((p - q).abs().max()) for p, q in zip(kernel_shade(), torch_shade())))

    # ---- 12 overlay frames on the per-class figure
    base = kernel_shade()[0]
    layout = {"size": [480, 640], "panels": [main_panel]}
    path = np.linspace(xy[classes == "a"].mean(0), xy[classes == "n"].mean(0), FRAMES)
    frames = [[{"panel": 0, "kind": "disc", "xy": p, "colour": figures.PATH_COLOUR}] for p in path]
    rows = [figures.marker_primitives(layout, f)[0] for f in frames]
    fx = torch.arange(640, device=dev, dtype=torch.float32)[None, :] + 0.5
    fy = torch.arange(480, device=dev, dtype=torch.float32)[:, None] + 0.5

    def torch_overlay():
        images = base.unsqueeze(0).repeat(FRAMES, 1, 1, 1)
        for i, q in enumerate(rows):
            cov = (float(q[7]) + 0.5 - torch.sqrt((fx - float(q[1])) ** 2 + (fy - float(q[2])) ** 2)).clamp(0, 1)
            cov = cov * ((fx >= q[12]) & (fx <= q[14]) & (fy >= q[13]) & (fy <= q[15]))
            w = float(q[11]) * cov
            images[i] = images[i] * (1 - w) + torch.tensor(q[8:11], device=dev)[:, None, None] * w
        return images

    a, b = median_pair(lambda: figures.overlay(base, layout, frames), torch_overlay, opts.repeats, opts.warmup)
    res.update(overlay_ms=a * 1e3, torch_overlay_ms=b * 1e3,
               overlay_max_diff=float((figures.overlay(base, layout, frames) - torch_overlay()).abs().max()))

    # ---- the whole figure set, files included
    with tempfile.TemporaryDirectory() as tmp:
        def whole():
            figures.embedding_figures(xy, classes, np.zeros(len(xy), bool), np.zeros(len(xy), bool), tmp,
                                      regions=regions, device=dev)
        whole()
        res["figure_set_s"] = statistics.median(wall(whole) for _ in range(3))

    res = {k: (float(f"{v:.3g}") if "diff" in k else round(v, 4)) if isinstance(v, float) else v
           for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
