"""``python tools/bench_evaluate.py [--out FILE]``: the evaluation harness on the
GPU, one JSON line, printed and written to ``profiles/evaluate_bench.json``
(or ``FILE``; ``--out ''`` only prints).

Kernel figures are the median of ``--repeats`` (>= 5) timed repeats of
``--calls`` back-to-back calls after a warm-up, wall clock around work that
ends in a device synchronise, at the traversal shape: 75 groups of 10 frames,
17 039 vertices, the template's 15 regions.

* ``group_errors_us`` / ``region_means_us``: ``ops.group_vertex_errors`` and
  ``ops.region_means`` (``csrc/evaluate.hip``), with the bytes they must move
  (``*_bytes``: every input element once, every output element once) and the
  rate that gives (``*_gbs``).
* ``composed_*_us``: the same results from what the package offered before,
  in the same run, alternating with the kernels: ``ops.vertex_errors`` on an
  expanded copy of every group's first frame (the copy included), and
  ``index_select`` + ``mean`` per region.  ``*_equal``: the results compared.
* ``traversal_s``, ``diversity_s``: ``Tester.latent_traversals(use_z_stats=False,
  animations=False)`` and ``Tester.compute_diversity(10000)`` over the golden
  weights, each on its own (median of ``--harness-repeats``).
* ``png_encode_s`` / ``apng_encode_s``: ``rendering.save_png`` of the tiled
  picture of 75 error maps and ``rendering.save_apng`` of the 900-frame
  animation of a whole traversal (host work: quantised frames in, file out).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

CONFIG = {
    "optimization": {"epochs": 1, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
}


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
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per timed kernel repeat")
    ap.add_argument("--harness-repeats", type=int, default=3)
    ap.add_argument("--diversity-samples", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.json"),
                    help="file that receives the line ('' = none)")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import evaluation, ops, precompute, rendering
    from craniofacialsd_vae_amd import manager as M

    if not torch.cuda.is_available():
        raise RuntimeError("bench_evaluate measures on the GPU; no GPU visible")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    npz = recipe.load_topology()
    groups, n, nv = 75, 10, int(npz["spiral_0"].shape[0])
    res = {"bench": "evaluate", "device": torch.cuda.get_device_name(0), "repeats": opts.repeats,
           "calls_per_repeat": opts.calls, "groups": groups, "frames_per_group": n, "vertices": nv}

    with tempfile.TemporaryDirectory() as tmp:
        precompute.write_ply(os.path.join(tmp, "template.ply"), npz["pos_0"], npz["face_0"], npz["template_colors"])
        os.makedirs(os.path.join(tmp, "pre"))
        np.savez(os.path.join(tmp, "pre", "topology.npz"), **npz)
        cfg = dict(CONFIG, data={"template_path": os.path.join(tmp, "template.ply"),
                                 "precomputed_path": os.path.join(tmp, "pre"), "normalize_data": True,
                                 "to_mm_constant": 89.11, "swap_features": True})
        man = M.ModelManager(cfg, device=dev, precomputed_storage_path=cfg["data"]["precomputed_path"],
                             use_graph=False)
        man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
        meshes = recipe.load_meshes()
        norm = {"mean": torch.from_numpy(meshes["norm_mean"]).float().contiguous(),
                "std": torch.from_numpy(meshes["norm_std"]).float().contiguous()}
        stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
        tester = evaluation.Tester(man, norm, None, None, os.path.join(tmp, "out"), cfg, latent_stats=stats)
        tester.set_renderings_size(256)
        tester.set_rendering_background_color([1, 1, 1])
        csr = man.topology.region_csr
        res.update(regions=csr.n_regions, region_entries=csr.nnz, longest_region=max(csr.lengths),
                   region_means_depth=ops.region_means_depth(max(csr.lengths)))

        # ---- the two kernels against the composed operators, on real traversal frames
        z = tester.traversal_latents(use_z_stats=False).reshape(groups * n, -1)
        frames = tester._unnormalize_verts(tester._decode(z)).contiguous()

        def composed_errors():
            first = frames.view(groups, n, nv, 3)[:, :1].expand(groups, n, nv, 3).reshape(groups * n, nv, 3)
            return ops.vertex_errors(frames, first.contiguous(), to_mm=89.11)

        def repeat(fn):
            def run():
                for _ in range(opts.calls):
                    fn()
            return run

        a, b = median_pair(repeat(lambda: ops.group_vertex_errors(frames, n, to_mm=89.11)), repeat(composed_errors),
                           opts.repeats, opts.warmup)
        nbytes = groups * n * nv * (12 + 4)
        res.update(group_errors_us=a / opts.calls * 1e6, composed_errors_us=b / opts.calls * 1e6,
                   group_errors_bytes=nbytes, group_errors_gbs=nbytes / (a / opts.calls) / 1e9)
        diffs = ops.group_vertex_errors(frames, n, to_mm=89.11)
        res["group_errors_equal"] = bool(torch.equal(diffs, composed_errors()))
        last = diffs.view(groups, n, nv)[:, -1].contiguous()
        lists = [csr.idx[csr.ptr_host[r]:csr.ptr_host[r + 1]].long() for r in range(csr.n_regions)]

        def composed_means():
            return torch.stack([last.index_select(1, lst).mean(1) for lst in lists], dim=1)

        a, b = median_pair(repeat(lambda: ops.region_means(last, csr)), repeat(composed_means), opts.repeats,
                           opts.warmup)
        nbytes = groups * csr.nnz * 4 + csr.nnz * 4 + groups * csr.n_regions * 4
        res.update(region_means_us=a / opts.calls * 1e6, composed_means_us=b / opts.calls * 1e6,
                   region_means_bytes=nbytes, region_means_gbs=nbytes / (a / opts.calls) / 1e9)
        ref = composed_means()
        res["region_means_max_rel_diff"] = float(((ops.region_means(last, csr) - ref).abs() / ref.abs()).max())

        # ---- the harness
        def med(fn, warm=1):
            for _ in range(warm):
                fn()
            return statistics.median(wall(fn) for _ in range(opts.harness_repeats))

        res["traversal_s"] = med(lambda: tester.latent_traversals(use_z_stats=False, animations=False))
        gen = torch.Generator()
        res["diversity_samples"] = opts.diversity_samples
        res["diversity_s"] = med(lambda: tester.compute_diversity(opts.diversity_samples, gen.manual_seed(1)))
        res["diversity_mm"] = tester.compute_diversity(opts.diversity_samples, gen.manual_seed(1))
        shots, maps = tester._traversal_pictures(frames, diffs, groups, n)
        tiled = rendering.make_grid(maps[:, -1], nrow=5, padding=10, pad_value=255).cpu()
        anim = torch.cat([shots, maps], dim=-1)
        anim = torch.cat([anim, torch.zeros_like(anim[:, :2])], dim=1).flatten(0, 1).cpu()
        res["apng_frames"] = int(anim.shape[0])
        res["png_encode_s"] = med(lambda: rendering.save_png(os.path.join(tmp, "t.png"), tiled), warm=0)
        res["apng_encode_s"] = med(lambda: rendering.save_apng(os.path.join(tmp, "t.apng"), anim, fps=4), warm=0)
        res["png_bytes"] = os.path.getsize(os.path.join(tmp, "t.png"))
        res["apng_bytes"] = os.path.getsize(os.path.join(tmp, "t.apng"))

    res = {k: (float(f"{v:.3g}") if "diff" in k else round(v, 6 if k.endswith("_s") else 3))
           if isinstance(v, float) else v for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
