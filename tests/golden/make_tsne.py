"""Writes ``tsne_sklearn.npz``: what scikit-learn 1.7.2's own t-SNE functions
give on small inputs, for ``tests/test_tsne_host.py`` and ``tests/test_gpu_tsne.py``
(which import no scikit-learn).  Run on the CPU: ``python tests/golden/make_tsne.py``.

1. Affinities: ``n = 200, d = 11`` random fp32 rows at perplexity 30 -- the
   neighbour indices and fp32 squared distances TSNE hands to
   ``_joint_probabilities_nn`` and the CSR ``P`` it returns.
2. Gradient: KL and gradient of ``_kl_divergence_bh(angle=0.0, compute_error=True)``
   for that ``P`` at two embeddings (``1e-4 * randn`` and ``5 * randn``).
3. Whole fits: ``kl_divergence_`` of ``TSNE(init='random', random_state=s)``
   for five seeds on ``tsne_oracle.clusters()``.
It also measures how far the float64 restatement ``tests/tsne_oracle.py`` is
from each of these (``gap_*``: the tests allow four times that) and prints the
figures DESIGN section 14 quotes.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.manifold import TSNE, _t_sne
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_oracle as O  # noqa: E402

PERPLEXITY, SEEDS = 30.0, (0, 1, 2, 3, 4)


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    rs = np.random.RandomState(11)
    z = rs.randn(200, 11).astype(np.float32)
    n = z.shape[0]
    k = min(n - 1, int(3.0 * PERPLEXITY + 1))
    nn = NearestNeighbors(algorithm="auto", n_neighbors=k, metric="euclidean").fit(z)
    dist = nn.kneighbors_graph(mode="distance")
    dist.data **= 2
    dist.sort_indices()
    nn_idx = dist.indices.reshape(n, k).astype(np.int32)
    nn_d2 = dist.data.reshape(n, k).astype(np.float32)
    p = _t_sne._joint_probabilities_nn(dist, PERPLEXITY, 0)
    p.sort_indices()
    out = {"z": z, "nn_idx": nn_idx, "nn_d2": nn_d2, "p_indptr": p.indptr.astype(np.int32),
           "p_indices": p.indices.astype(np.int32), "p_data": p.data.astype(np.float64)}

    p_cond, _ = O.perplexity_search(nn_d2, PERPLEXITY)
    dense = O.symmetrize(nn_idx, p_cond)
    row_ptr, col, val = O.to_csr(dense)
    assert np.array_equal(row_ptr, p.indptr) and np.array_equal(col, p.indices), "sparsity pattern differs"
    out["gap_p"] = np.abs(val - p.data).max() / p.data.max()

    gaps_grad, gaps_kl = [], []
    for name, scale in (("small", 1e-4), ("large", 5.0)):
        y = (scale * rs.randn(n, 2)).astype(np.float32)
        kl, grad = _t_sne._kl_divergence_bh(y.ravel(), p.copy(), 1.0, n, 2, angle=0.0, compute_error=True,
                                            num_threads=1)
        out[f"y_{name}"], out[f"kl_{name}"], out[f"grad_{name}"] = y, np.float64(kl), grad.reshape(n, 2)
        okl, ograd = O.kl_and_grad(p.toarray(), y)
        gaps_grad.append(np.abs(ograd - grad.reshape(n, 2)).max() / np.abs(ograd).max())
        gaps_kl.append(abs(okl - kl) / abs(okl))
    out["gap_grad"], out["gap_kl"] = max(gaps_grad), max(gaps_kl)

    x, label = O.clusters()
    out["fit_x"], out["fit_label"] = x, label.astype(np.int32)
    kls, nn_ok = [], []
    for s in SEEDS:
        t = TSNE(n_components=2, init="random", random_state=s, perplexity=PERPLEXITY)
        emb = t.fit_transform(x)
        kls.append(t.kl_divergence_)
        near, _ = O.knn(emb, 1)
        nn_ok.append(float((label[near[:, 0]] == label).mean()))
    out["fit_kl"], out["fit_seeds"] = np.array(kls), np.array(SEEDS)
    np.savez_compressed(os.path.join(HERE, "tsne_sklearn.npz"), **out)
    print(f"gap_p {out['gap_p']:.3e}  gap_grad {out['gap_grad']:.3e}  gap_kl {out['gap_kl']:.3e}")
    print(f"TSNE kl_divergence_ {np.round(kls, 4).tolist()}  nearest-neighbour label agreement {nn_ok}")
    if "--restatement" in sys.argv:  # the float64 loop on the same P, for DESIGN section 14 (about a minute)
        fx_idx, fx_d2 = O.knn(x, k)
        fp = O.symmetrize(fx_idx, O.perplexity_search(fx_d2.astype(np.float32), PERPLEXITY)[0])
        res = []
        for s in SEEDS:
            y0 = 1e-4 * np.random.RandomState(s).standard_normal((x.shape[0], 2)).astype(np.float32)
            emb, kl, it = O.fit(fp, y0)
            near, _ = O.knn(emb, 1)
            res.append((round(float(kl), 4), it, float((label[near[:, 0]] == label).mean())))
        print("restatement (kl, n_iter, nn agreement):", res)


if __name__ == "__main__":
    main()
