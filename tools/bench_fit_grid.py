"""``python tools/bench_fit_grid.py``: the Chamfer search of a fit against a
DENSE scan, brute force (``ops.nn_points``) against the exact uniform grid
(``ops.nn_points_grid``), one JSON line (kept as
``profiles/fit_grid_bench.json``).

The scans are demo mesh 5 (``tests/golden``) at its own size and
midpoint-subdivided once, twice and three times in this tool (17 039, about
68 k, 272 k and 1.09 M vertices), each with its vertices permuted as
``bench_fit.py`` permutes them; the generated side is 16 decoded heads
(``[16, 17 039, 3]``).  Per size, HIP events around back-to-back calls after a
warm-up of the same shapes:

* ``brute_gen_to_scan_us`` / ``brute_scan_to_gen_us``: one ``ops.nn_points``
  call per direction (``--brute-iters`` calls; a direction is 16 x 17 039 x P
  pairs);
* ``grid_gen_to_scan_us`` / ``grid_scan_to_gen_us``: one ``ops.nn_points_grid``
  call per direction against grids built beforehand -- the heads against the
  scan's grid, the scan's points (in the Morton order of its ``PointGrid``,
  results in file order) against the 16 heads' grids;
* ``gen_grid_build_us``: the per-call build of the 16 generated-head grids
  (cell ids, stable sort, cell table and records), which a fit pays every
  iteration; ``scan_grid_build_us``: the scan's, paid once per fit (Morton
  order included);
* ``evaluated_gen_to_scan`` / ``evaluated_scan_to_gen``: the mean number of
  points evaluated per query (brute force evaluates P and 17 039);
* ``bit_identical_*``: ``torch.equal`` of distances AND indices with brute
  force, per direction;
* ``fit_iteration_brute_us`` / ``fit_iteration_grid_us``: one iteration of
  ``fitting.fit_points`` (16 starts, ``--fit-iters`` iterations, total time /
  iterations: the scan's grid build and the closing error evaluation
  included), alternating the two searches, the second pass kept; and
  ``fit_bit_identical``: the two fits return equal latents and histories.

``--sweep`` measures instead, per ``--points-per-cell`` candidate of the
``cells=None`` rule (``ops.default_grid_cells``), what a fit iteration pays
for the search: both grid directions plus the generated grids' build
(``profiles/fit_grid_sweep.json``).  ``--points-per-cell C`` runs the main
measurement with that constant instead of the committed one.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def subdivide(verts, faces):
    """One midpoint subdivision: every edge gets a vertex, every triangle
    becomes four.  ``verts`` ``[V, 3]`` float, ``faces`` ``[F, 3]`` int64; the
    first V vertices of the result are the old ones."""
    import torch
    nv = verts.shape[0]
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = e.min(1).values * nv + e.max(1).values
    uniq, inv = torch.unique(key, return_inverse=True)
    mid = (verts[uniq // nv] + verts[uniq % nv]) * 0.5
    nf = faces.shape[0]
    m01, m12, m20 = (inv[:nf] + nv), (inv[nf:2 * nf] + nv), (inv[2 * nf:] + nv)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    new = torch.cat([torch.stack([a, m01, m20], 1), torch.stack([b, m12, m01], 1), torch.stack([c, m20, m12], 1),
                     torch.stack([m01, m12, m20], 1)])
    return torch.cat([verts, mid]), new


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--levels", type=int, default=3, help="subdivisions of the largest scan")
    ap.add_argument("--iters", type=int, default=20, help="timed calls of the grid search")
    ap.add_argument("--brute-iters", type=int, default=3, help="timed calls of the brute-force search")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--points-per-cell", type=float, default=None)
    ap.add_argument("--sweep", default=None, metavar="C,C,...",
                    help="candidates of the cells=None constant, e.g. 1,2,4,8,16,32")
    opts = ap.parse_args(argv)

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import fitting, ops
    from craniofacialsd_vae_amd import model as M

    if not torch.cuda.is_available():
        raise RuntimeError("bench_fit_grid measures on the GPU; none visible")
    dev = "cuda"
    if opts.points_per_cell is not None:
        ops.NN_GRID_POINTS_PER_CELL = float(opts.points_per_cell)
    npz = recipe.load_topology()
    n_lv = int(npz["n_levels"])
    spirals = [torch.from_numpy(np.asarray(npz[f"spiral_{l}"], np.int64)).to(dev) for l in range(n_lv)]

    def sp(name, l):
        idx = np.stack([npz[f"{name}_{l}_row"], npz[f"{name}_{l}_col"]]).astype(np.int64)
        return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(np.asarray(npz[f"{name}_{l}_val"], np.float32)),
                                       tuple(np.asarray(npz[f"{name}_{l}_shape"]).tolist())).to(dev)

    net = M.Model(3, recipe.OUT_CH, recipe.LATENT, spirals, [sp("down", l) for l in range(n_lv)],
                  [sp("up", l) for l in range(n_lv)], is_vae=True).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    meshes = recipe.load_meshes()
    mean = torch.from_numpy(meshes["norm_mean"]).float().to(dev)
    std = torch.from_numpy(meshes["norm_std"]).float().to(dev)
    g = torch.Generator().manual_seed(0)
    bsz = opts.starts
    with torch.no_grad():
        x = (net.decode(torch.randn(bsz, recipe.LATENT, generator=g).to(dev)) * std + mean).contiguous()
    nv = x.shape[1]
    verts = torch.from_numpy(meshes["verts"][5].astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.asarray(npz["face_0"], np.int64).reshape(-1, 3)).to(dev)
    lidx = recipe.sample_idx(nv, k=12, seed=3).tolist()
    lnd = verts[lidx].contiguous()
    scans = []
    for level in range(opts.levels + 1):
        if level:
            verts, faces = subdivide(verts, faces)
        perm = torch.randperm(verts.shape[0], generator=torch.Generator().manual_seed(2)).to(dev)
        scans.append(verts[perm].contiguous()[None])

    def search_us(y):
        """What one fit iteration pays for the grid search against scan y."""
        ygrid = ops.PointGrid(y)
        xgrid = ops.PointGrid(x, queries=False)
        t = timed(lambda: ops.nn_points_grid(x, ygrid), opts.iters, opts.warmup)
        t += timed(lambda: ops.nn_points_grid(ygrid, xgrid), opts.iters, opts.warmup)
        return t + timed(lambda: ops.PointGrid(x, queries=False), opts.iters, opts.warmup)

    if opts.sweep:
        cands = [float(c) for c in opts.sweep.split(",")]
        table, cells = {}, {}
        for c in cands:
            ops.NN_GRID_POINTS_PER_CELL = c
            table[c] = [round(search_us(y), 1) for y in scans]
            cells[c] = [ops.default_grid_cells(int(p))[0] for p in [nv] + [y.shape[1] for y in scans]]
        # the constant is chosen for the dense sizes the feature exists for: the two largest
        score = {c: sum(table[c][i] / min(table[k][i] for k in cands) for i in (-2, -1)) for c in cands}
        best = min(cands, key=lambda c: score[c])
        out = {"starts": bsz, "gen_points": nv, "scan_points": [int(y.shape[1]) for y in scans],
               "grid_search_us": {f"{c:g}": table[c] for c in cands},
               "cells_gen_and_scans": {f"{c:g}": cells[c] for c in cands},
               "best_points_per_cell": best, "iters": opts.iters}
        print(json.dumps(out))
        return out

    out = {"starts": bsz, "gen_points": nv, "points_per_cell": ops.NN_GRID_POINTS_PER_CELL, "iters": opts.iters,
           "brute_iters": opts.brute_iters, "fit_iters": opts.fit_iters,
           "gen_cells": ops.default_grid_cells(nv)[0], "sizes": []}
    for y in scans:
        p = int(y.shape[1])
        row = {"scan_points": p, "scan_cells": ops.default_grid_cells(p)[0]}
        row["scan_grid_build_us"] = round(timed(lambda: ops.PointGrid(y), 3, 1), 1)
        row["gen_grid_build_us"] = round(timed(lambda: ops.PointGrid(x, queries=False), opts.iters, opts.warmup), 1)
        ygrid, xgrid = ops.PointGrid(y), ops.PointGrid(x, queries=False)
        for key, brute, grid in (("gen_to_scan", lambda: ops.nn_points(x, y), lambda: ops.nn_points_grid(x, ygrid)),
                                 ("scan_to_gen", lambda: ops.nn_points(y, x), lambda: ops.nn_points_grid(ygrid, xgrid))):
            d0, i0 = brute()
            d1, i1, count = (ops.nn_points_grid(x, ygrid, return_stats=True) if key == "gen_to_scan"
                             else ops.nn_points_grid(ygrid, xgrid, return_stats=True))
            row[f"bit_identical_{key}"] = bool(torch.equal(d0, d1) and torch.equal(i0, i1))
            row[f"evaluated_{key}"] = round(float(count.double().mean()), 2)
            del d0, i0, d1, i1, count
            row[f"brute_{key}_us"] = round(timed(brute, opts.brute_iters, 1), 1)
            row[f"grid_{key}_us"] = round(timed(grid, opts.iters, opts.warmup), 1)
        del ygrid, xgrid

        def fit(search):
            return fitting.fit_points(net.decode, y[0], lnd, lidx, mean, std, torch.zeros(recipe.LATENT), n_starts=bsz,
                                      iterations=opts.fit_iters, seed=1, search=search)

        for _ in range(2):  # alternate the two loops: the second pass is the one kept
            row["fit_iteration_brute_us"] = round(timed(lambda: fit("brute"), 1, 0) / opts.fit_iters, 1)
            row["fit_iteration_grid_us"] = round(timed(lambda: fit("grid"), 1, 0) / opts.fit_iters, 1)
        row["fit_speedup"] = round(row["fit_iteration_brute_us"] / row["fit_iteration_grid_us"], 2)
        a, b = fit("brute"), fit("grid")
        row["fit_bit_identical"] = bool(all(torch.equal(getattr(a, n), getattr(b, n)) for n in
                                            ("z_all", "verts", "errors_shape", "chamfer_history", "landmark_history")))
        row["bit_identical"] = row["bit_identical_gen_to_scan"] and row["bit_identical_scan_to_gen"]
        del a, b
        out["sizes"].append(row)
    out["bit_identical"] = all(r["bit_identical"] and r["fit_bit_identical"] for r in out["sizes"])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
