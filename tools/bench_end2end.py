"""``python tools/bench_end2end.py [--out FILE]``: what the classifier head
(``classifier.mlp_training_type: end2end``) adds to the replayed training step,
one JSON line, printed and written to ``profiles/end2end_bench.json`` (or
``FILE``; ``--out ''`` only prints).

Two runners of ``step.TrainStep`` live in ONE process, on the craniofacial
shapes (bs 4 -> 16 swapped meshes of 17 039 vertices, latent 75, fp32): the
default step, and the step with an ``MLPClassifier(75, [512, 128, 64], 3)``
attached (``SDVAEEngine.attach_classifier_head``).  Each is captured once; a
timed repeat is ``--steps`` steps through ``TrainStep.run`` (the multi-step
graph), wall clock around work that ends in a device synchronise.  The two
runners alternate, the order flipping every repeat, after ``--warmup``
untimed repeats of both.

* ``plain_ms`` / ``head_ms``: the median ms per step of each runner over
  ``--repeats`` (>= 5) repeats; ``*_min`` / ``*_max``: their spread.
* ``delta_us``: ``head_ms - plain_ms`` in microseconds (the two launches the
  head adds); ``launches_plain`` / ``launches_head``: libcfsd calls per step.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=800, help="steps per timed repeat")
    ap.add_argument("--dataset", type=int, default=256, help="resident synthetic meshes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "end2end_bench.json"),
                    help="file that receives the line ('' = none)")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import _abi, topology
    from craniofacialsd_vae_amd import classify as C
    from craniofacialsd_vae_amd import engine as E
    from craniofacialsd_vae_amd.step import TrainStep

    if not torch.cuda.is_available():
        raise RuntimeError("bench_end2end measures on the GPU; no GPU visible")
    dev = torch.device("cuda", 0)
    topo = topology.DeviceTopology.from_npz(recipe.load_topology(), device=dev)
    weights = {k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()}
    g = torch.Generator().manual_seed(0)
    base = torch.from_numpy(recipe.normalized_meshes(12))
    meshes = (base[torch.arange(opts.dataset) % 12] + 0.01 * torch.randn(opts.dataset, *base.shape[1:], generator=g))
    meshes = meshes.to(dev)
    hidden, n_classes = [512, 128, 64], 3

    def runner(head):
        eng = E.SDVAEEngine(topo, E.ModelSpec(), swap_bs=4, device=dev)
        eng.load_state_dict(weights)
        data = E.ResidentData(meshes, bs=4, shuffle=True, class_idx=np.arange(opts.dataset) % n_classes)
        if head:
            mlp = C.MLPClassifier(75, hidden, n_classes, device=dev, seed=0, lr=1e-4)
            eng.attach_classifier_head(mlp, torch.tensor([0.2, 0.5, 0.3]), 1.0)
        ts = TrainStep(eng, data)
        with _abi.trace_launches() as rec:  # one eager step: the calls a step makes
            ts.step()
        torch.cuda.synchronize(dev)
        ts.capture()
        return eng, ts, len(rec)

    plain = runner(False)
    head = runner(True)

    def timed(ts):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ts.run(opts.steps)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / opts.steps * 1e3

    for _ in range(opts.warmup):
        timed(plain[1])
        timed(head[1])
    tp, th = [], []
    for r in range(opts.repeats):
        for ts, out in ((plain[1], tp), (head[1], th)) if r % 2 == 0 else ((head[1], th), (plain[1], tp)):
            out.append(timed(ts))
    for eng, _, _ in (plain, head):
        eng.check_health()
    res = {"bench": "end2end", "device": torch.cuda.get_device_name(0), "repeats": opts.repeats,
           "steps_per_repeat": opts.steps, "batch_size": 4, "step_rows": 16, "mlp_dims": [75] + hidden + [n_classes],
           "steps_per_graph": plain[1].steps_per_graph,
           "plain_ms": statistics.median(tp), "plain_ms_min": min(tp), "plain_ms_max": max(tp),
           "head_ms": statistics.median(th), "head_ms_min": min(th), "head_ms_max": max(th),
           "delta_us": (statistics.median(th) - statistics.median(tp)) * 1e3,
           "launches_plain": plain[2], "launches_head": head[2],
           "classification_loss_mean": float(head[0].cls_acc[0].item() / max(head[0].cls_acc[2].item(), 1.0)),
           "losses_finite": bool(torch.isfinite(head[0].loss_acc).all() and torch.isfinite(head[0].cls_acc).all())}
    res = {k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
