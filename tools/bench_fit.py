"""``python tools/bench_fit.py``: the latent-fitting hot path on the GPU, one
JSON line.

Measured at the craniofacial size (B = 16 starts, N = P = 17 039 points: the
decoded heads against a permuted decode), HIP events around ``--iters``
back-to-back calls after ``--warmup`` calls:

* ``nn_gen_to_target_us`` / ``nn_target_to_gen_us``: one ``ops.nn_points``
  call per direction (queries [16, N, 3] vs one shared target; the shared
  target's points vs 16 reference sets);
* ``valu_peak_fraction``: the useful arithmetic of the search -- 8 FLOP per
  point pair (3 subtractions, 3 products, 2 additions) -- over the measured
  time, as a share of the MI355X's 157.3 TFLOP/s fp32 vector peak (the
  compare / select work of the arg-min is not counted as useful);
* ``cdist_*_us``: the same search as chunked ``torch.cdist(...).min(-1)`` on
  the same device in the same process (the only alternative without these
  kernels; ``--cdist-chunk`` batch elements per [chunk, N, P] matrix), and
  ``cdist_index_agreement``, the share of queries where it picks the same
  index (cdist uses the |q|^2 + |r|^2 - 2 q.r expansion);
* ``fit_iteration_us``: ``fitting.fit_points`` over the drop-in Model with 16
  starts, total time / iterations (the closing error evaluation included);
* ``decode_fwd_bwd_us``: the decoder forward + data-gradient backward alone
  (what an iteration spends outside the Chamfer search and Adam).

``--surface`` measures the point-to-triangle search instead (the line kept as
``profiles/fit_surface_bench.json``): the scan is demo mesh 5 with its
vertices permuted and the template's faces re-indexed (P = 17 039 vertices,
33 737 triangles), the generated side the same 16 decoded heads:

* ``pf_gen_to_scan_{cull,brute}_us`` / ``pf_scan_to_gen_{cull,brute}_us``: one
  ``ops.point_face_distance`` call per direction with culling on and off (the
  culled call includes its seed: the gather of the referenced vertices and
  ``ops.nn_points`` over them, timed alone as ``seed_*_us``; towards the scan
  the per-face records are kept in an ``ops.SurfaceMesh``, towards the heads
  every call includes the pre-launch that writes them); the scan's vertices
  query in the Morton order of ``SurfaceMesh.queries``, as the fit uses them,
  and ``scan_file_order_to_gen`` repeats the culled search in the permuted
  file order (a wave's 64 queries are then scattered over the head);
* ``groups_entered_*`` / ``faces_evaluated_*``: of the culled search, the
  share of (wave, group) and (wave, face) pairs that pass the sphere tests;
* ``pairs_per_us_*_brute``: point-triangle pairs per microsecond of the
  brute-force walk (every pair evaluated: the price of one full test);
* ``surface_fit_iteration_us`` and ``vertex_fit_iteration_us``: one iteration
  of ``fitting.fit_points`` with and without the faces, in this process.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

FP32_VECTOR_PEAK = 157.3e12  # FLOP/s, MI355X spec
FLOP_PER_PAIR = 8


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


def surface_main(opts, net, mean, std, x, dev):
    """The ``--surface`` line (see the module docstring)."""
    import numpy as np
    import torch

    import recipe
    from craniofacialsd_vae_amd import fitting, ops

    bsz, nv = x.shape[0], x.shape[1]
    g = torch.Generator().manual_seed(2)
    gf = torch.from_numpy(np.asarray(recipe.load_topology()["face_0"], np.int32).reshape(-1, 3)).to(dev)
    full = torch.from_numpy(recipe.load_meshes()["verts"][5].astype(np.float32)).to(dev)
    perm = torch.randperm(nv, generator=g).to(dev)  # scan vertex j = demo vertex perm[j]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(nv, device=dev)
    scan, sf = full[perm].contiguous()[None], inv[gf.long()].to(torch.int32).contiguous()
    lidx = recipe.sample_idx(nv, k=12, seed=3).tolist()
    lnd = full[lidx].contiguous()
    mesh = ops.SurfaceMesh(scan, sf)
    nf, ngroups = int(gf.shape[0]), (int(gf.shape[0]) + ops.PF_GROUP - 1) // ops.PF_GROUP
    out = {"starts": bsz, "points": nv, "faces": nf, "iters": opts.iters, "brute_iters": opts.brute_iters}
    gen_ref = ops.face_table(gf, nv).ref_idx
    for key, pts, verts, faces in (("gen_to_scan", x, mesh, None), ("scan_to_gen", mesh.queries, x, gf),
                                   ("scan_file_order_to_gen", scan, x, gf)):
        on = ops.point_face_distance(pts, verts, faces, cull=True, return_stats=True)
        off = ops.point_face_distance(pts, verts, faces, cull=False)
        if not all(torch.equal(a, b) for a, b in zip(on[:3], off)):
            raise RuntimeError(f"{key}: the culled search differs from brute force")
        waves = on[3].shape[0]
        out[f"groups_entered_{key}"] = round(int(on[3][:, 0].sum()) / (waves * ngroups), 4)
        out[f"faces_evaluated_{key}"] = round(int(on[3][:, 1].sum()) / (waves * nf), 4)
        out[f"pf_{key}_cull_us"] = round(timed(lambda: ops.point_face_distance(pts, verts, faces), opts.iters,
                                               opts.warmup), 1)
        if key == "scan_file_order_to_gen":
            continue
        us = timed(lambda: ops.point_face_distance(pts, verts, faces, cull=False), opts.brute_iters, 1)
        out[f"pf_{key}_brute_us"] = round(us, 1)
        out[f"pairs_per_us_{key}_brute"] = round(float(bsz) * nv * nf / us, 1)
        if faces is None:
            seed = lambda: ops.nn_points(pts, mesh.ref)  # noqa: E731
        else:
            seed = lambda: ops.nn_points(pts, verts.index_select(1, gen_ref).contiguous())  # noqa: E731
        out[f"seed_{key}_us"] = round(timed(seed, opts.iters, opts.warmup), 1)

    def fit(**kw):
        return fitting.fit_points(net.decode, scan[0], lnd, lidx, mean, std, torch.zeros(recipe.LATENT), n_starts=bsz,
                                  iterations=opts.fit_iters, seed=1, **kw)

    for _ in range(2):  # alternate the two loops: the second pass is the one kept
        out["surface_fit_iteration_us"] = round(
            timed(lambda: fit(target_faces=sf, template_faces=gf), 1, 1) / opts.fit_iters, 1)
        out["vertex_fit_iteration_us"] = round(timed(fit, 1, 1) / opts.fit_iters, 1)
    res = fit(target_faces=sf, template_faces=gf)
    out["fit_iters"] = opts.fit_iters
    out["surface_term_first_last"] = [float(res.chamfer_history[0]), float(res.chamfer_history[-1])]
    out["surface_distance_best"] = float(res.surface_mm)
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fit-iters", type=int, default=50)
    ap.add_argument("--cdist-iters", type=int, default=5)
    ap.add_argument("--cdist-chunk", type=int, default=2)
    ap.add_argument("--surface", action="store_true", help="measure the point-to-triangle search instead")
    ap.add_argument("--brute-iters", type=int, default=3)
    opts = ap.parse_args(argv)

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import fitting, ops
    from craniofacialsd_vae_amd import model as M

    if not torch.cuda.is_available():
        raise RuntimeError("bench_fit measures on the GPU; none visible")
    dev = "cuda"
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
        full = net.decode(0.5 * torch.randn(1, recipe.LATENT, generator=g).to(dev))[0] * std + mean
    nv = x.shape[1]
    y = full[torch.randperm(nv, generator=g).to(dev)].contiguous()[None]
    lidx = recipe.sample_idx(nv, k=12, seed=3).tolist()
    lnd = full[lidx].contiguous()
    if opts.surface:
        return surface_main(opts, net, mean, std, x, dev)

    out = {"starts": bsz, "points": nv, "iters": opts.iters}
    pairs = float(bsz) * nv * nv
    for key, q, r in (("gen_to_target", x, y), ("target_to_gen", y, x)):
        us = timed(lambda: ops.nn_points(q, r), opts.iters, opts.warmup)
        out[f"nn_{key}_us"] = round(us, 1)
        out[f"valu_peak_fraction_{key}"] = round(pairs * FLOP_PER_PAIR / (us * 1e-6) / FP32_VECTOR_PEAK, 4)

    ch = max(1, min(opts.cdist_chunk, bsz))

    def cdist_nn(q, r):
        d, i = [], []
        for s in range(0, bsz, ch):
            qq = q[s:s + ch] if q.shape[0] > 1 else q.expand(min(ch, bsz - s), -1, -1)
            rr = r[s:s + ch] if r.shape[0] > 1 else r.expand(min(ch, bsz - s), -1, -1)
            m = torch.cdist(qq, rr).min(-1)
            d.append(m.values)
            i.append(m.indices)
        return torch.cat(d) ** 2, torch.cat(i)

    for key, q, r in (("gen_to_target", x, y), ("target_to_gen", y, x)):
        out[f"cdist_{key}_us"] = round(timed(lambda: cdist_nn(q, r), opts.cdist_iters, 1), 1)
        out[f"speedup_{key}"] = round(out[f"cdist_{key}_us"] / out[f"nn_{key}_us"], 2)
    out["cdist_index_agreement"] = round(
        float((cdist_nn(x, y)[1] == ops.nn_points(x, y)[1].long()).float().mean().item()), 6)
    out["cdist_chunk"] = ch

    def fit():
        return fitting.fit_points(net.decode, y[0], lnd, lidx, mean, std, torch.zeros(recipe.LATENT), n_starts=bsz,
                                  iterations=opts.fit_iters, seed=1)

    out["fit_iteration_us"] = round(timed(fit, 1, 1) / opts.fit_iters, 1)
    out["fit_iters"] = opts.fit_iters

    z = torch.randn(bsz, recipe.LATENT, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(bsz, nv, 3, generator=g).to(dev)

    def dec():
        z.grad = None
        (net.decode(z) * w).sum().backward()

    with fitting.frozen(net):
        out["decode_fwd_bwd_us"] = round(timed(dec, opts.iters, opts.warmup), 1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
