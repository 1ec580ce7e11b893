"""``python tools/bench_render.py``: the rendering path on the GPU, one JSON
line (kept as ``profiles/render_bench.json``).

Measured on 16 heads (the 12 demo meshes of ``tests/golden/demo_meshes.npz``
and the first four again) with the template's 33 737 triangles, HIP events
around ``--iters`` back-to-back calls after ``--warmup`` calls:

* ``project_us``: ``ops.project_vertices`` without shading (view transform);
* ``gouraud_vertices_us``: the same launch with normals and vertex colours;
* ``raster_256_us`` / ``raster_512_us``: ``ops.rasterize_ndc`` alone (face
  records + raster + outputs, no image), and ``covered_share_256``;
* ``render_256_us`` / ``render_512_us``: the whole ``rendering.render``
  (Gouraud, grey 0.5) at 256 x 256 and 512 x 512;
* ``render_errors_256_us``: the shadeless error-map rendering
  (``errors_to_colors`` + render);
* ``log_images_ms``: one ``ModelManager.log_images`` of 16 meshes (decoder
  forward, three renderings each, the grid, the PNG file), wall clock.
"""
import argparse
import json
import os
import sys
import tempfile
import time

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--heads", type=int, default=16)
    opts = ap.parse_args(argv)

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import manager as M
    from craniofacialsd_vae_amd import ops, precompute, rendering

    dev = torch.device("cuda", 0)
    topo, m = recipe.load_topology(), recipe.load_meshes()
    idx = [i % len(m["verts"]) for i in range(opts.heads)]
    verts = torch.from_numpy(m["verts"][idx].astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.asarray(topo["face_0"], np.int32).reshape(-1, 3)).to(dev)
    cam = rendering.look_at()
    res = {"bench": "render", "heads": opts.heads, "vertices": int(verts.shape[1]), "faces": int(faces.shape[0]),
           "iters": opts.iters, "device": torch.cuda.get_device_name(0)}

    res["project_us"] = timed(lambda: ops.project_vertices(verts, cam), opts.iters, opts.warmup)
    res["gouraud_vertices_us"] = timed(lambda: ops.project_vertices(verts, cam, faces, shade=True), opts.iters,
                                       opts.warmup)
    ndc, vz, _ = ops.project_vertices(verts, cam)
    for size in (256, 512):
        res[f"raster_{size}_us"] = timed(lambda: ops.rasterize_ndc(ndc, vz, faces, size, cam.znear), opts.iters,
                                         opts.warmup)
        res[f"render_{size}_us"] = timed(lambda: rendering.render(verts, faces, image_size=size), opts.iters,
                                         opts.warmup)
    res["covered_share_256"] = (ops.rasterize_ndc(ndc, vz, faces, 256, cam.znear)[0] >= 0).float().mean().item()
    errors = torch.rand(verts.shape[:2], device=dev) * 6

    def error_map():
        return rendering.render(verts, faces, rendering.errors_to_colors(errors, 0, 5), shading="none")

    res["render_errors_256_us"] = timed(error_map, opts.iters, opts.warmup)

    with tempfile.TemporaryDirectory() as d:
        precompute.write_ply(os.path.join(d, "template.ply"), topo["pos_0"], topo["face_0"], topo["template_colors"])
        os.makedirs(os.path.join(d, "pre"))
        np.savez(os.path.join(d, "pre", "topology.npz"), **topo)
        cfg = {"optimization": {"epochs": 1, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                                "kl_weight": 1e-4, "latent_consistency_weight": 0.5},
               "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
                         "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
                         "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
               "data": {"template_path": os.path.join(d, "template.ply"), "precomputed_path": os.path.join(d, "pre"),
                        "normalize_data": True, "to_mm_constant": 89.11, "swap_features": True}}
        man = M.ModelManager(cfg, device=dev, precomputed_storage_path=cfg["data"]["precomputed_path"],
                             use_graph=False)
        man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
        norm = {"mean": torch.from_numpy(m["norm_mean"].astype(np.float32)).to(dev),
                "std": torch.from_numpy(m["norm_std"].astype(np.float32)).to(dev)}
        x = ((verts - norm["mean"]) / norm["std"]).contiguous()
        out = os.path.join(d, "renderings")
        for _ in range(2):
            man.log_images(x, out, 0, norm)
        torch.cuda.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for e in range(reps):
            path = man.log_images(x, out, e, norm)
        torch.cuda.synchronize()
        res["log_images_ms"] = (time.perf_counter() - t0) * 1e3 / reps
        res["log_images_png_bytes"] = os.path.getsize(path)
    res = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
