"""``python tools/bench_classify.py``: the classifier stage on the GPU, one
JSON line (kept as ``profiles/classify_bench.json``).

Every figure is the median of ``--repeats`` (>= 5) timed repeats after a
warm-up, wall clock around work that ends in a device synchronise.

* ``mlp_*``: one training epoch of the MLP classifier at the craniofacial
  shape (``[75, 512, 128, 64, 4]``, batch 4, ``--rows`` synthetic latents:
  rows / 4 steps) through ``MLPClassifier.run_epoch`` (libcfsd: two launches
  per step, one library call per epoch), and the same module trained with
  PyTorch eager on the same device in the same process (``nn.Sequential``,
  ``CrossEntropyLoss(weight)``, ``torch.optim.Adam``, one ``.item()`` pair per
  step as ``mlp_classifier_epoch`` reads them); the two are timed in
  alternating order.  ``mlp_forward_us``: one ``cfsd_mlp_fwd`` over all rows.
* ``stats_*`` / ``scores_*``: ``ops.class_stats`` and
  ``ops.discriminant_scores`` (QDA: one whitening per class) at ``--n`` rows,
  d = 75, 4 classes, and over the full region set (15 windows of d = 5 of the
  same buffer), against on-device torch: ``index_add_`` statistics (means,
  then centred outer products through one batched matmul per class) and
  batched-matmul scoring.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4096, help="latents of the MLP epoch")
    ap.add_argument("--n", type=int, default=50000, help="rows of the discriminant benchmark")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed discriminant repeat")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import torch
    import torch.nn as nn

    import cfsd_loader
    cfsd_loader.load()
    from craniofacialsd_vae_amd import classify as C
    from craniofacialsd_vae_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    dims, bs, n_cls = [75, 512, 128, 64, 4], 4, 4
    res = {"bench": "classify", "device": torch.cuda.get_device_name(0), "repeats": opts.repeats,
           "mlp_dims": dims, "mlp_batch": bs, "mlp_rows": opts.rows, "mlp_steps_per_epoch": opts.rows // bs,
           "n": opts.n, "d": 75, "classes": n_cls, "regions": 15, "calls_per_repeat": opts.calls}

    # ---- MLP training epoch
    z = torch.randn(opts.rows, dims[0], generator=g).to(dev)
    y = torch.randint(0, n_cls, (opts.rows,), generator=g, dtype=torch.int32).to(dev)
    w = torch.full((n_cls,), 1.0 / n_cls, device=dev)
    mlp = C.MLPClassifier(dims[0], dims[1:-1], dims[-1], device=dev, seed=0, lr=1e-4)
    layers = []
    for i in range(1, len(dims)):
        layers += [nn.Linear(dims[i - 1], dims[i]), nn.ReLU()]
    eager = nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(eager.parameters(), lr=1e-4, weight_decay=0.0)
    crit = nn.CrossEntropyLoss(w)
    yl = y.long()

    def eager_epoch():
        loss_sum = acc_sum = 0.0
        for t in range(opts.rows // bs):
            zb, yb = z[t * bs:(t + 1) * bs], yl[t * bs:(t + 1) * bs]
            opt.zero_grad()
            out = eager(zb)
            lab = torch.max(torch.log_softmax(out, dim=1), dim=1)[1]
            loss = crit(out, yb)
            acc = 100 * torch.sum(lab == yb) / bs
            loss.backward()
            opt.step()
            loss_sum += loss.item()
            acc_sum += acc.item()
        return loss_sum, acc_sum

    t_hip, t_eager = median_pair(lambda: mlp.run_epoch(z, y, w, bs, train=True), eager_epoch, opts.repeats,
                                 opts.warmup)
    steps = opts.rows // bs
    res.update(mlp_epoch_s=t_hip, mlp_step_us=t_hip / steps * 1e6, eager_epoch_s=t_eager,
               eager_step_us=t_eager / steps * 1e6, mlp_speedup=t_eager / t_hip)
    for _ in range(opts.warmup):
        mlp(z)
    res["mlp_forward_us"] = statistics.median(wall(lambda: mlp(z)) for _ in range(opts.repeats)) * 1e6

    # ---- statistics and scores
    n, d = opts.n, 75
    zz = torch.randn(n, d, generator=g).to(dev)
    yy = torch.randint(0, n_cls, (n,), generator=g, dtype=torch.int32).to(dev)
    yyl = yy.long()
    windows = [(5 * r, 5) for r in range(15)]

    def torch_stats(cols):
        x = zz[:, cols[0]:cols[0] + cols[1]]
        count = torch.zeros(n_cls, device=dev).index_add_(0, yyl, torch.ones(n, device=dev))
        mean = torch.zeros(n_cls, cols[1], device=dev).index_add_(0, yyl, x) / count[:, None]
        xc = x - mean[yyl]
        onehot = torch.nn.functional.one_hot(yyl, n_cls).to(xc.dtype)            # [n, C]
        scatter = torch.einsum("nc,na,nb->cab", onehot, xc, xc)
        return count, mean, scatter

    def torch_scores(x, mean, whiten, offset):
        y_ = torch.matmul((x[None] - mean[:, None]), whiten)                      # [C, n, d]
        sc = -0.5 * (y_ * y_).sum(-1).T + offset
        return sc, sc.argmax(1)

    def repeat(fn):
        def run():
            for _ in range(opts.calls):
                fn()
        return run

    full = (0, d)
    ws = torch.empty(int(ops._abi.lib().cfsd_class_stats_workspace(n, d, n_cls)) // 4 + 1, device=dev)
    a, b = median_pair(repeat(lambda: ops.class_stats(zz, yy, n_cls, full, workspace=ws)),
                       repeat(lambda: torch_stats(full)), opts.repeats, opts.warmup)
    res.update(stats_us=a / opts.calls * 1e6, torch_stats_us=b / opts.calls * 1e6)
    a, b = median_pair(repeat(lambda: [ops.class_stats(zz, yy, n_cls, c, workspace=ws) for c in windows]),
                       repeat(lambda: [torch_stats(c) for c in windows]), opts.repeats, opts.warmup)
    res.update(stats_regions_us=a / opts.calls * 1e6, torch_stats_regions_us=b / opts.calls * 1e6)

    def fitted(cols):
        count, mean, scatter = ops.class_stats(zz, yy, n_cls, cols)
        f = C.finish_qda(count.cpu().numpy(), mean.cpu().double().numpy(), scatter.cpu().double().numpy())
        return tuple(torch.as_tensor(f[k], dtype=torch.float32).to(dev).contiguous()
                     for k in ("means", "whiten", "offset"))

    q_full = fitted(full)
    q_reg = [fitted(c) for c in windows]
    a, b = median_pair(repeat(lambda: ops.discriminant_scores(zz, *q_full, cols=full)),
                       repeat(lambda: torch_scores(zz, *q_full)), opts.repeats, opts.warmup)
    res.update(scores_us=a / opts.calls * 1e6, torch_scores_us=b / opts.calls * 1e6)
    a, b = median_pair(
        repeat(lambda: [ops.discriminant_scores(zz, *q, cols=c) for q, c in zip(q_reg, windows)]),
        repeat(lambda: [torch_scores(zz[:, c[0]:c[0] + c[1]], *q) for q, c in zip(q_reg, windows)]),
        opts.repeats, opts.warmup)
    res.update(scores_regions_us=a / opts.calls * 1e6, torch_scores_regions_us=b / opts.calls * 1e6)
    # the two paths compute the same thing
    sc = ops.discriminant_scores(zz, *q_full, cols=full)["scores"]
    ref = torch_scores(zz, *q_full)[0]
    res["scores_max_rel_diff"] = float((sc - ref).abs().max() / ref.abs().max())
    s_hip, s_ref = ops.class_stats(zz, yy, n_cls, full)[2], torch_stats(full)[2]
    res["stats_max_rel_diff"] = float((s_hip - s_ref).abs().max() / s_ref.abs().max())

    res = {k: (float(f"{v:.3g}") if "diff" in k else round(v, 6 if k.endswith("_s") else 3))
           if isinstance(v, float) else v for k, v in res.items()}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
