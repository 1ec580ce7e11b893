"""``python tools/bench_planning.py [--out FILE]``: the surgical-planning stage
on the GPU, one JSON line, printed and written to
``profiles/planning_bench.json`` (or ``FILE``; ``--out ''`` only prints).

Kernel figures are the median of ``--repeats`` (>= 5) timed repeats after a
warm-up, wall clock around work that ends in a device synchronise, each
alternating in the same run with the same result composed from what the
package offered before.

* ``plan_targets_us``: ``ops.plan_targets`` (``csrc/planning.hip``) for 256
  patients at ``L = 75``, ``steps = 5000``, three levels (``--calls``
  back-to-back calls per repeat).  ``composed_targets_us``: per patient the
  ``[5000, 75]`` grid from torch operators on the device, times ``whiten`` in
  float64, ``<=`` and ``argmax`` per level (one pass over the 256 patients per
  repeat).  ``plan_targets_index_equal``: the fraction of equal indices.
* ``pair_metrics_us``: ``ops.pair_metrics`` for 256 pairs times 16 windows (the
  whole latent and 15 regions of 5).  ``composed_pairs_us``: per window three
  ``ops.discriminant_scores`` calls (pre, post, displacement) and torch norms.
  ``pair_metrics_max_rel_diff``: the two compared (fp32 against float64 sums).
* ``plan_patient_s``: one whole ``Tester.interpolate_syndrome_to_normal`` with
  11 procedures over the golden weights (12 groups of 11 frames decoded,
  rendered twice at 512 pixels and written; median of ``--harness-repeats``),
  and ``plan_to_normal_us``, its planning arithmetic alone
  (``Tester.plan_to_normal``: the mask upload and the two launches).
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
    "classifier": {"main_model_type": "qda", "mlp_training_type": "after", "mlp_hidden_features": [32, 16],
                   "mlp_lr": 1e-3, "mlp_epochs": 1},
}
LEVELS, STEPS, N = (3.0, 2.0, 1.0), 5000, 256


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
    ap.add_argument("--calls", type=int, default=50, help="back-to-back kernel calls per timed repeat")
    ap.add_argument("--harness-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planning_bench.json"),
                    help="file that receives the line ('' = none)")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import numpy as np
    import torch

    import cfsd_loader
    import classify_cases
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import classify, evaluation, ops, precompute
    from craniofacialsd_vae_amd import manager as M

    if not torch.cuda.is_available():
        raise RuntimeError("bench_planning measures on the GPU; no GPU visible")
    dev = torch.device("cuda", 0)
    res = {"bench": "planning", "device": torch.cuda.get_device_name(0), "repeats": opts.repeats,
           "calls_per_repeat": opts.calls, "patients": N, "latent": 75, "steps": STEPS, "levels": len(LEVELS)}

    def repeat(fn):
        def run():
            for _ in range(opts.calls):
                fn()
        return run

    # ---- the seeded classifier case: a QDA per window, fitted on the device
    case = classify_cases.make_case("full75")
    z_train, y_train = torch.from_numpy(case["z"]).to(dev), torch.from_numpy(case["y"]).to(dev)
    z = torch.from_numpy(case["zt"][:N]).to(dev).contiguous()
    cols = [(0, 75)] + [(5 * r, 5) for r in range(15)]
    qdas = [classify.QuadraticDiscriminant(dev).fit(z_train, y_train, cols=c, n_classes=4) for c in cols]
    mean, whiten = qdas[0]._mean[0].contiguous(), qdas[0]._whiten[0].contiguous()
    whiten64, steps_i = whiten.double(), torch.arange(STEPS, device=dev, dtype=torch.float32)[:, None]

    def composed_targets():
        out = []
        for p in range(N):
            step = (mean - z[p]) / float(STEPS - 1)
            grid = torch.where(steps_i < STEPS // 2, z[p] + step * steps_i, mean - step * (STEPS - 1 - steps_i))
            maha2 = (((grid - mean).double() @ whiten64) ** 2).sum(1)
            out.append(torch.stack([(maha2 <= lv * lv).int().argmax() for lv in LEVELS]))
        return torch.stack(out)

    a, b = median_pair(repeat(lambda: ops.plan_targets(z, mean, whiten, LEVELS, STEPS)), composed_targets,
                       opts.repeats, opts.warmup)
    res.update(plan_targets_us=a / opts.calls * 1e6, composed_targets_us=b * 1e6)
    index = ops.plan_targets(z, mean, whiten, LEVELS, STEPS)[1]
    res["plan_targets_index_equal"] = float((index.long() == composed_targets()).double().mean())

    # ---- 256 pairs x 16 windows
    pre, post = z, torch.from_numpy(case["zt"][:N][::-1].copy()).to(dev).contiguous()
    windows, n_mean, n_whiten = [], 0, 0
    for (col0, d) in cols:
        windows.append((col0, d, n_mean, n_whiten))
        n_mean, n_whiten = n_mean + d, n_whiten + d * d
    p_mean = torch.cat([q._mean[0] for q in qdas]).contiguous()
    p_whiten = torch.cat([q._whiten[0].reshape(-1) for q in qdas]).contiguous()
    zero = torch.zeros(1, device=dev)

    def composed_pairs():
        out = []
        for (col0, d), q in zip(cols, qdas):
            m, w = q._mean[:1].contiguous(), q._whiten[:1].contiguous()
            shifted = (post - pre).contiguous()
            shifted[:, col0:col0 + d] += m[0]
            md = [torch.sqrt(ops.discriminant_scores(t, m, w, zero, (col0, d), want_maha2=True, want_scores=False,
                                                     want_pred=False)["maha2"][:, 0]) for t in (pre, post, shifted)]
            a_, b_ = pre[:, col0:col0 + d] - m, post[:, col0:col0 + d] - m
            v = b_ - a_
            cos = (v * -a_).sum(1) / (v.norm(dim=1) * a_.norm(dim=1))
            out.append(torch.stack([md[0], md[1], a_.norm(dim=1), b_.norm(dim=1), cos, md[2]], dim=1))
        return torch.stack(out, dim=1)

    a, b = median_pair(repeat(lambda: ops.pair_metrics(pre, post, windows, p_mean, p_whiten)), composed_pairs,
                       opts.repeats, opts.warmup)
    res.update(pairs=N, windows=len(windows), pair_metrics_us=a / opts.calls * 1e6, composed_pairs_us=b * 1e6)
    raw, ref = ops.pair_metrics(pre, post, windows, p_mean, p_whiten), composed_pairs()
    res["pair_metrics_max_rel_diff"] = float(((raw - ref).abs() / ref.abs().clamp_min(1e-3)).max())

    # ---- one whole patient over the golden weights
    with tempfile.TemporaryDirectory() as tmp:
        npz = recipe.load_topology()
        precompute.write_ply(os.path.join(tmp, "template.ply"), npz["pos_0"], npz["face_0"], npz["template_colors"])
        os.makedirs(os.path.join(tmp, "pre"))
        os.makedirs(os.path.join(tmp, "meshes"))
        np.savez(os.path.join(tmp, "pre", "topology.npz"), **npz)
        meshes = recipe.load_meshes()
        rs = np.random.RandomState(3)
        names, verts = [], []
        for i in range(40):
            v = meshes["verts"][i % 12] + (0 if i < 12 else rs.normal(0, 0.002, meshes["verts"][0].shape))
            names.append(f"{'nacm'[i % 4]}_{i:03d}.obj")
            verts.append(v.astype(np.float32))
            with open(os.path.join(tmp, "meshes", names[-1]), "w") as f:
                for p in verts[-1]:
                    f.write("v %.9g %.9g %.9g\n" % tuple(p))
        cfg = dict(CONFIG, data={"template_path": os.path.join(tmp, "template.ply"),
                                 "precomputed_path": os.path.join(tmp, "pre"),
                                 "dataset_path": os.path.join(tmp, "meshes"), "normalize_data": True,
                                 "to_mm_constant": 89.11, "swap_features": True})
        man = M.ModelManager(cfg, device=dev, precomputed_storage_path=cfg["data"]["precomputed_path"],
                             use_graph=False)
        man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
        norm = {"mean": torch.from_numpy(meshes["norm_mean"]).float().contiguous(),
                "std": torch.from_numpy(meshes["norm_std"]).float().contiguous()}
        zs = man.encode(((torch.from_numpy(np.stack(verts)) - norm["mean"]) / norm["std"]).to(dev).contiguous())
        ys = torch.tensor(man.class2idx([n[0] for n in names]), dtype=torch.int32)
        man.lda.fit(zs, ys, n_classes=4)
        man.qda.fit(zs, ys, n_classes=4)
        for key, (lo, hi) in man.latent_regions.items():
            man.region_ldas[key].fit(zs, ys, cols=(lo, hi - lo), n_classes=4)
            man.region_qdas[key].fit(zs, ys, cols=(lo, hi - lo), n_classes=4)
        keys = [str(k) for k in man.latent_regions]
        cfg["planning"] = {"procedures": {f"procedure_{i}": [keys[i], keys[i + 1]] for i in range(11)}}
        stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
        tester = evaluation.Tester(man, norm, None, None, os.path.join(tmp, "out"), cfg, latent_stats=stats)
        patient = os.path.join(tmp, "meshes", names[1])

        def med(fn, warm=1):
            for _ in range(warm):
                fn()
            return statistics.median(wall(fn) for _ in range(opts.harness_repeats))

        res["procedures"] = 11
        res["plan_patient_s"] = med(lambda: tester.interpolate_syndrome_to_normal(patient))
        z_p = tester._load_and_encode(patient)
        res["plan_to_normal_us"] = med(repeat(lambda: tester.plan_to_normal(z_p))) / opts.calls * 1e6

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
