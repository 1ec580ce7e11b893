"""``python tools/bench_tsne.py [--out FILE] [--sizes N,N,..]``: t-SNE on the GPU,
one JSON line, printed and written to ``profiles/tsne_bench.json`` (or
``FILE``; ``--out ''`` only prints).

Per size ``n`` (``d = 75``, 16 Gaussian clusters, perplexity 30), medians of
``--repeats`` timed repeats after a warm-up, wall clock around work that ends
in a device synchronise:

* ``knn_ms`` / ``affinities_ms``: ``ops.knn_rows`` (k = 91) and
  ``ops.tsne_affinities``, one call per repeat.
* ``step_us``: one iteration, ``ops.tsne_step`` (three launches) -- ``--calls``
  back-to-back iterations per repeat, divided by their number.
  ``torch_step_us``: the yardstick, the same arithmetic composed from torch
  operators on the same device (dense ``n x n`` ``q`` through one matrix
  product for the distances and one for the forces, the sparse attraction
  through ``index_select`` / ``index_add_``), alternating with the kernels in
  the same run.  ``slower_than_torch`` lists the sizes where the HIP median is
  not below torch's.  ``grad_gap``: the two gradients compared (of max |grad|).
* ``pair_rate``: pairs per second of the iteration (``n^2 / step``; the
  repulsive kernel is all but a few per cent of it at the larger sizes) and
  ``valu_fraction``: that rate over the VALU bound of the repulsive kernel's
  inner loop priced from its ISA: per 32 pairs 208 full-rate vector
  instructions at 4 cycles and 32 ``v_rcp_f32`` at 8, 34 cycles per pair and
  wave, on 256 CUs x 4 SIMDs x 64 lanes at 2.4 GHz = 4.6e12 pairs/s.
* ``fit_s``: the wall clock of a whole 1000-iteration ``tsne.fit_transform``
  (kNN and affinities included), once; ``fit_kl``, ``fit_n_iter``.
* ``sklearn_fit_s``: scikit-learn's ``TSNE`` (Barnes-Hut, angle 0.5, its
  default) on the host for sizes up to ``--sklearn-max-n``, where it imports;
  null otherwise.  Context only.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

VALU_BOUND_PAIRS_PER_S = 256 * 4 * 64 * 2.4e9 / 34.0


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


def latents(n, d, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    centres = 3.0 * torch.randn(16, d, generator=g)
    return (centres[torch.arange(n) % 16] + torch.randn(n, d, generator=g)).cuda()


def torch_step(y, update, gains, row, col, val, momentum, lr):
    """One iteration from torch operators; returns the gradient."""
    import torch
    sq = (y * y).sum(1)
    q = 1.0 / (1.0 + (sq[:, None] + sq[None, :] - 2.0 * (y @ y.t())).clamp_(min=0.0))
    q.fill_diagonal_(0.0)
    z = q.sum()
    q2 = q * q
    rep = q2.sum(1, keepdim=True) * y - q2 @ y
    diff = y.index_select(0, row) - y.index_select(0, col)
    pq = val / (1.0 + (diff * diff).sum(1))
    attr = torch.zeros_like(y).index_add_(0, row, pq[:, None] * diff)
    grad = 4.0 * (attr - rep / z)
    inc = update * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    update.mul_(momentum).sub_(lr * gains * grad)
    y.add_(update)
    return grad


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back iterations per timed repeat")
    ap.add_argument("--sklearn-max-n", type=int, default=2048)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    opts = ap.parse_args(argv)

    import torch

    import cfsd_loader
    cfsd_loader.load()
    from craniofacialsd_vae_amd import ops, tsne

    line = {"bench": "tsne", "d": 75, "perplexity": 30.0, "device": torch.cuda.get_device_name(0), "sizes": {},
            "slower_than_torch": [], "valu_bound_pairs_per_s": VALU_BOUND_PAIRS_PER_S}
    for n in [int(s) for s in opts.sizes.split(",") if s]:
        z = latents(n, 75, n)
        k = min(n - 1, 91)
        res = {"k": k, "splits": ops.tsne_splits(n)}
        knn = [wall(lambda: ops.knn_rows(z, k)) for _ in range(opts.warmup + opts.repeats)][opts.warmup:]
        _, d2 = ops.knn_rows(z, k)
        aff = [wall(lambda: ops.tsne_affinities(d2, 30.0)) for _ in range(opts.warmup + opts.repeats)][opts.warmup:]
        res["knn_ms"], res["affinities_ms"] = statistics.median(knn) * 1e3, statistics.median(aff) * 1e3
        csr = ops.tsne_joint_probabilities(z, 30.0)
        row = torch.repeat_interleave(torch.arange(n, device="cuda"), (csr[0][1:] - csr[0][:-1]).long())
        col = csr[1].long()
        res["nnz"] = int(col.numel())
        y0 = (5.0 * torch.randn(n, 2, generator=torch.Generator().manual_seed(1))).cuda()
        lr = max(n / 12.0 / 4.0, 50.0)
        state = [[y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)] for _ in range(2)]
        ws, grad = ops.tsne_workspace(n, 0, "cuda"), torch.empty_like(y0)
        calls = opts.calls if n <= 8192 else max(3, opts.calls // 4)
        g_hip = ops.tsne_step(y0.clone(), torch.zeros_like(y0), torch.ones_like(y0), csr, 0.8, lr).clone()
        g_torch = torch_step(y0.clone(), torch.zeros_like(y0), torch.ones_like(y0), row, col, csr[2], 0.8, lr)
        res["grad_gap"] = ((g_hip - g_torch).abs().max() / g_torch.abs().max()).item()
        del g_hip, g_torch

        def hip():
            for _ in range(calls):
                ops.tsne_step(*state[0], csr, 0.8, lr, workspace=ws, grad=grad)

        def composed():
            for _ in range(calls):
                torch_step(*state[1], row, col, csr[2], 0.8, lr)

        t_hip, t_torch = median_pair(hip, composed, opts.repeats, opts.warmup)
        res["step_us"], res["torch_step_us"] = t_hip / calls * 1e6, t_torch / calls * 1e6
        res["pair_rate"] = n * n / (t_hip / calls)
        res["valu_fraction"] = res["pair_rate"] / VALU_BOUND_PAIRS_PER_S
        if not res["step_us"] < res["torch_step_us"]:
            line["slower_than_torch"].append(n)
        torch.cuda.empty_cache()
        if not opts.no_fit:
            out = {}
            res["fit_s"] = wall(lambda: out.update(fit=tsne.fit_transform(z, generator=torch.Generator().manual_seed(0))))
            res["fit_kl"], res["fit_n_iter"] = out["fit"].kl_divergence, out["fit"].n_iter
        res["sklearn_fit_s"] = None
        if n <= opts.sklearn_max_n:
            try:
                from sklearn.manifold import TSNE
                x = z.cpu().numpy()
                t0 = time.perf_counter()
                TSNE(n_components=2, init="random", random_state=0, n_jobs=16).fit_transform(x)
                res["sklearn_fit_s"] = time.perf_counter() - t0
            except ImportError:
                pass
        line["sizes"][str(n)] = res
        print(f"# n {n}: {json.dumps(res)}", file=sys.stderr, flush=True)
    text = json.dumps(line)
    print(text)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
