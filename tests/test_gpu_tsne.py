"""t-SNE on the GPU (``csrc/tsne.hip``, ``ops.knn_rows`` / ``tsne_affinities`` /
``tsne_step``, ``tsne.fit_transform``, ``Tester.tsne_embeddings``).

Reference: ``tsne_oracle.py``, the float64 restatement of scikit-learn 1.7.2's
``TSNE(method='barnes_hut', angle=0)`` that ``test_tsne_host.py`` pins on
scikit-learn's own results, and those results themselves
(``golden/tsne_sklearn.npz``) for the whole fit.

Shapes: ``n`` one below, at and one above every exported tile constant
(``CFSD_TSNE_KNN_ROWS`` 16, ``_KNN_COLS`` / ``_KNN_DIMS`` 64, ``_ATT_ROWS`` 16,
``_TILE`` 128, ``_LONG_ROW`` 256, ``_ROWS`` 512), ``n = k + 1``, ``d`` in {1, 3,
75, 512} and around the 64-coordinate chunk, ``k`` in {1, 16, 91}.

Bounds.  kNN on integers: exact.  kNN on floats: ``d * 2^-23`` relative (d
coordinates, the running sum rounded twice for each, 2^-24 a time).  Affinities: the
search's own 1e-5 exit plus 1e-5 for the fp32 rounding of the outputs.  One
step: 1e-5 of max |grad| (the project's fp32 kernel bar) for the gradient, 1e-5
relative for KL, 1e-6 for the update rule restated on the device's own
gradient (a handful of fp32 operations per coordinate, 2^-24 each).
"""
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe

pytestmark = pytest.mark.gpu
cfsd_loader.load()
from craniofacialsd_vae_amd import evaluation, ops, tsne  # noqa: E402

import tsne_oracle as O  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_sklearn.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


# ---------------------------------------------------------------- kNN
# (n, d, k): around the 16-row, 64-column and 64-coordinate tiles, n = k + 1, the issue's d and k
KNN_CASES = [(2, 1, 1), (15, 3, 1), (16, 3, 15), (17, 75, 16), (63, 1, 16), (64, 63, 16), (65, 64, 16), (66, 65, 1),
             (92, 3, 91), (129, 512, 91), (200, 75, 91), (257, 3, 16)]


@pytest.mark.parametrize("n,d,k", KNN_CASES)
def test_knn_rows_exact_on_integers(n, d, k):
    """Integer coordinates in [-8, 8]: every d2 is exact in fp32 and ties are
    everywhere; idx and d2 equal the (d2, index) top-k of an int64 brute force.
    A tenth of the rows are copies of others (d2 = 0)."""
    rs = np.random.RandomState(n * 1000 + d)
    z = rs.randint(-8, 9, size=(n, d))
    dup = rs.choice(n, max(1, n // 10), replace=False)
    z[dup] = z[rs.randint(0, n, size=dup.size)]
    ref_idx, ref_d2 = O.knn(z, k)
    idx, d2 = ops.knn_rows(torch.from_numpy(z.astype(np.float32)).to(DEV), k)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (n, k)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), ref_d2)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ref_idx)
    assert (ref_d2[:, 0] == 0).any() or n < 10


@pytest.mark.parametrize("n,d,k", KNN_CASES)
def test_knn_rows_random_floats(n, d, k):
    """Each d2 within d * 2^-23 relative of the float64 distance of its idx,
    rows ascending, self excluded, no index twice, and no row left out whose
    float64 distance is below the row's largest by more than that bound."""
    g = torch.Generator().manual_seed(n * 1000 + d)
    z = torch.randn(n, d, generator=g) * torch.tensor([1.0, 30.0, 0.01, 5.0])[torch.arange(n) % 4, None]
    idx, d2 = ops.knn_rows(z.to(DEV), k)
    idx, d2 = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)
    z64 = z.numpy().astype(np.float64)
    full = ((z64[:, None, :] - z64[None, :, :]) ** 2).sum(-1)
    tol = d * 2.0 ** -23
    assert (idx >= 0).all() and (idx < n).all() and (idx != np.arange(n)[:, None]).all()
    assert all(len(set(r)) == k for r in idx)
    true = np.take_along_axis(full, idx, axis=1)
    gap = np.abs(d2 - true) / true
    print(f"n {n} d {d} k {k}: d2 max rel err {gap.max():.3e} (bound {tol:.3e})")
    assert (np.abs(d2 - true) <= tol * true).all()
    assert (np.diff(d2, axis=1) >= 0).all()
    out = np.ones((n, n), bool)
    out[np.arange(n)[:, None], idx] = False
    np.fill_diagonal(out, False)
    worst = true.max(axis=1, keepdims=True)
    assert not (out & (full < worst * (1 - tol))).any()


def test_knn_rows_refuses_bad_arguments():
    z = torch.zeros(10, 3, device=DEV)
    for k in (0, 10, ops.TSNE_MAX_K + 1):
        with pytest.raises(ValueError):
            ops.knn_rows(z, k)
    with pytest.raises(ValueError):
        ops.knn_rows(torch.zeros(10, 513, device=DEV), 2)
    with pytest.raises(ValueError):
        ops.knn_rows(torch.zeros(1, 3, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.knn_rows(z.double(), 2)


# ---------------------------------------------------------------- affinities
def _affinity_inputs(kind):
    g = torch.Generator().manual_seed(5)
    if kind == "gaussian":
        return torch.randn(300, 11, generator=g), 30.0
    if kind == "scales":  # four clusters of very different scale
        scale = torch.tensor([1e-3, 1.0, 40.0, 3e3])[torch.arange(260) % 4, None]
        return torch.randn(260, 7, generator=g) * scale + scale * 10, 30.0
    base = torch.randn(50, 5, generator=g)  # every row four times: three neighbours at d2 = 0
    return base.repeat(4, 1), 10.0


@pytest.mark.parametrize("kind", ["gaussian", "scales", "duplicates"])
def test_tsne_affinities(kind):
    """Rows of p_cond sum to 1 within 1e-6; their float64 entropy is within
    2e-5 of log(perplexity); p_cond is the float64 softmax at the returned
    beta within 1e-5 relative (an fp32 subnormal cannot hold a relative bound:
    the smallest normal, 1.2e-38, is allowed on top)."""
    z, perplexity = _affinity_inputs(kind)
    n = z.shape[0]
    k = min(n - 1, int(3 * perplexity + 1))
    _, d2 = ops.knn_rows(z.to(DEV), k)
    p_cond, beta = ops.tsne_affinities(d2, perplexity)
    assert p_cond.shape == (n, k) and beta.shape == (n,) and p_cond.dtype == beta.dtype == torch.float32
    p, b, dd = p_cond.cpu().numpy().astype(np.float64), beta.cpu().numpy().astype(np.float64), \
        d2.cpu().numpy().astype(np.float64)
    assert np.isfinite(p).all() and (p >= 0).all() and (b > 0).all()
    sums, ent = p.sum(1), O.entropy(p)
    e = np.exp(-dd * b[:, None])
    soft = e / e.sum(1, keepdims=True)
    rel = np.abs(p - soft) / np.maximum(soft, 1e-300)
    print(f"{kind}: |sum - 1| {np.abs(sums - 1).max():.2e}, |H - log perp| {np.abs(ent - np.log(perplexity)).max():.2e}, "
          f"softmax rel {rel[soft > 1e-30].max():.2e}, beta {b.min():.3g}..{b.max():.3g}")
    assert np.abs(sums - 1).max() <= 1e-6
    assert np.abs(ent - np.log(perplexity)).max() <= 2e-5
    assert (np.abs(p - soft) <= 1e-5 * soft + 1.2e-38).all()
    p2, b2 = ops.tsne_affinities(d2, perplexity)
    assert torch.equal(p2, p_cond) and torch.equal(b2, beta)


def test_tsne_joint_probabilities_matches_sklearn(gold):
    """kNN -> affinities -> symmetrise on the golden rows: scikit-learn's
    pattern, values within 1e-5 of max P (fp32 outputs of a float64 search that
    stops within 1e-5 of the same entropy)."""
    row_ptr, col, val = ops.tsne_joint_probabilities(torch.from_numpy(gold["z"]).to(DEV), 30.0)
    assert np.array_equal(row_ptr.cpu().numpy(), gold["p_indptr"]) and np.array_equal(col.cpu().numpy(), gold["p_indices"])
    gap = np.abs(val.cpu().numpy() - gold["p_data"]).max() / gold["p_data"].max()
    print(f"P vs scikit-learn: {gap:.3e} of max P")
    assert gap <= 1e-5
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        ops.tsne_joint_probabilities(torch.zeros(10, 3, device=DEV), 10.0)


# ---------------------------------------------------------------- one step
def _hub_csr(n, rs):
    """A P whose row 0 has n - 1 entries: every point names the hub (point 0,
    the centre of four clusters) and up to four other neighbours."""
    k = min(n - 1, 5)
    idx = np.zeros((n, k), np.int64)
    for i in range(n):
        others = np.delete(np.arange(1, n), i - 1) if i else np.arange(1, n)
        pick = rs.choice(others, k - (1 if i else 0), replace=False)
        idx[i] = np.concatenate([[0], pick]) if i else pick
    p = rs.rand(n, k) + 0.05
    p /= p.sum(1, keepdims=True)
    return ops.tsne_symmetrize(torch.from_numpy(idx.astype(np.int32)).to(DEV), torch.from_numpy(p.astype(np.float32)).to(DEV))


def _embedding(n, scale, rs):
    """Four clusters around the hub at the origin; points 1 and 2 coincide."""
    centres = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.float64)[np.arange(n) % 4]
    y = scale * (2.0 * centres + rs.randn(n, 2))
    y[0] = 0.0
    if n > 2:
        y[2] = y[1]
    return y.astype(np.float32)


def _check_step(csr, n, rs, exaggeration=1.0):
    dense = O.from_csr(*(t.cpu().numpy() for t in csr), n=n)
    momentum, lr = 0.8, 200.0
    for scale in (1e-4, 5.0):
        y0 = _embedding(n, scale, rs)
        u0 = (scale * 0.1 * rs.randn(n, 2)).astype(np.float32)
        k0 = rs.choice([0.01, 0.012, 0.8, 1.0, 2.2], size=(n, 2)).astype(np.float32)
        kl_ref, grad_ref = O.kl_and_grad(dense, y0, exaggeration)
        scale_g = np.abs(grad_ref).max()
        if n == 2:  # two points: attr = rep / Z = q (y_0 - y_1) / 2, the gradient is identically 0 and the
            diff = y0[0].astype(np.float64) - y0[1]  # bar is 1e-5 of the term that cancels, 4 attr
            scale_g = np.abs(4.0 * exaggeration * dense[0, 1] / (1.0 + (diff ** 2).sum()) * diff).max()
        runs = {}
        for splits in (1, 3, 0):
            for rep in range(2):
                y, u, k = (torch.from_numpy(a.copy()).to(DEV) for a in (y0, u0, k0))
                grad, result = ops.tsne_step(y, u, k, csr, momentum, lr, exaggeration=exaggeration, splits=splits,
                                             want_error=True)
                out = tuple(t.cpu() for t in (y, u, k, grad, result))
                if rep:
                    assert all(torch.equal(a, b) for a, b in zip(out, runs[splits])), "two calls differ"
                runs[splits] = out
            y1, u1, k1, grad, result = (t.numpy().astype(np.float64) for t in runs[splits])
            gap_g = np.abs(grad - grad_ref).max() / scale_g
            # two points: q / Z = p = 1/2, KL is identically 0 -- the bar is then 1e-5 of the two
            # terms that cancel, (sum p) log Z and sum p log(p / q), each about log 2 or larger
            gap_kl = abs(result[0] - kl_ref) / (abs(kl_ref) if n > 2 else exaggeration * np.log(2.0))
            ry, ru, rk, rnorm = O.update_rule(y0, u0, k0, grad, momentum, lr)
            gaps = [np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in ((y1, ry), (u1, ru), (k1, rk))]
            gap_n = abs(result[1] - rnorm) / rnorm
            print(f"n {n} scale {scale:g} splits {splits}: grad {gap_g:.2e} of max, KL {gap_kl:.2e} rel "
                  f"({result[0]:.6f}), update rule {max(gaps):.2e}, norm {gap_n:.2e}")
            assert gap_g <= 1e-5
            assert gap_kl <= 1e-5
            assert max(gaps) <= 1e-6 and gap_n <= 1e-6
            # without the error request: the same bits
            y, u, k = (torch.from_numpy(a.copy()).to(DEV) for a in (y0, u0, k0))
            g2 = ops.tsne_step(y, u, k, csr, momentum, lr, exaggeration=exaggeration, splits=splits)
            assert all(torch.equal(a.cpu(), b) for a, b in zip((y, u, k, g2), runs[splits][:4]))
        for splits in (3, 0):  # another grouping of the same sums: the same bar
            assert np.abs(runs[splits][3].numpy() - runs[1][3].numpy()).max() <= 1e-5 * scale_g
    return runs


@pytest.mark.parametrize("n", [2, 15, 16, 17, 127, 128, 129, 256, 257, 258, 511, 512, 513, 700])
def test_tsne_step_hub(n):
    """A hub row of n - 1 entries (below, at and above CFSD_TSNE_LONG_ROW: n =
    256, 257, 258), coincident points, embeddings of scale 1e-4 and 5, splits
    1 / 3 / auto."""
    rs = np.random.RandomState(n)
    csr = _hub_csr(n, rs)
    assert int(csr[0][1]) == n - 1
    _check_step(csr, n, rs)


def test_tsne_step_golden_p(gold):
    """scikit-learn's own P (n = 200) at the golden embeddings: the device
    gradient and KL against the oracle (bars above) and, for the record,
    against scikit-learn's fp32 _kl_divergence_bh."""
    n = gold["z"].shape[0]
    csr = tuple(torch.from_numpy(a).to(DEV) for a in (gold["p_indptr"], gold["p_indices"],
                                                      gold["p_data"].astype(np.float32)))
    _check_step(csr, n, np.random.RandomState(1))
    _check_step(csr, n, np.random.RandomState(2), exaggeration=12.0)
    for name in ("small", "large"):
        y, u, k = torch.from_numpy(gold[f"y_{name}"]).to(DEV), torch.zeros(n, 2, device=DEV), torch.ones(n, 2, device=DEV)
        grad, result = ops.tsne_step(y, u, k, csr, 0.5, 50.0, want_error=True)
        gap_g = np.abs(grad.cpu().numpy() - gold[f"grad_{name}"]).max() / np.abs(gold[f"grad_{name}"]).max()
        gap_kl = abs(result[0].item() - gold[f"kl_{name}"]) / gold[f"kl_{name}"]
        print(f"{name}: vs scikit-learn grad {gap_g:.2e} of max, KL {gap_kl:.2e} rel")
        assert gap_g <= 1e-5 + 4 * gold["gap_grad"] and gap_kl <= 1e-5 + 4 * gold["gap_kl"]


def test_tsne_step_refuses_bad_arguments():
    n = 10
    y, u, k = torch.zeros(n, 2, device=DEV), torch.zeros(n, 2, device=DEV), torch.ones(n, 2, device=DEV)
    csr = _hub_csr(n, np.random.RandomState(0))
    for bad in ({"splits": -1}, {"splits": ops.TSNE_MAX_SPLITS + 1}, {"exaggeration": 0.0},
                {"workspace": torch.zeros(4, device=DEV)}):
        with pytest.raises((ValueError, RuntimeError)):
            ops.tsne_step(y, u, k, csr, 0.5, 50.0, **bad)
    with pytest.raises(ValueError):
        ops.tsne_step(y, u[:5], k, csr, 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.tsne_step(y, u, k, (csr[0][:-1], csr[1], csr[2]), 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.tsne_step(y, u, k, (csr[0], csr[1].long(), csr[2]), 0.5, 50.0)


# ---------------------------------------------------------------- the whole fit
def test_fit_transform_clusters(gold):
    """Four Gaussian clusters of 150 points, d = 33: the final KL is at most
    scikit-learn's largest of five seeds plus twice their spread, every
    point's nearest neighbour in the embedding has its own label, n_iter <=
    1000, and the same seed gives the same bits."""
    x, label = torch.from_numpy(gold["fit_x"]).to(DEV), gold["fit_label"]
    bound = gold["fit_kl"].max() + 2 * (gold["fit_kl"].max() - gold["fit_kl"].min())
    fit = tsne.fit_transform(x, generator=torch.Generator().manual_seed(0))
    y = fit.y.cpu().numpy()
    near, _ = O.knn(y, 1)
    agree = (label[near[:, 0]] == label).mean()
    print(f"KL {fit.kl_divergence:.4f} (scikit-learn {gold['fit_kl'].min():.4f}..{gold['fit_kl'].max():.4f}, "
          f"bound {bound:.4f}), n_iter {fit.n_iter}, nearest-neighbour label agreement {agree:.4f}")
    assert fit.y.shape == (600, 2) and fit.y.is_cuda and np.isfinite(y).all()
    assert fit.kl_divergence <= bound
    assert agree == 1.0
    assert fit.n_iter <= 1000
    again = tsne.fit_transform(x, generator=torch.Generator().manual_seed(0))
    assert torch.equal(again.y, fit.y) and again.kl_divergence == fit.kl_divergence and again.n_iter == fit.n_iter
    given = tsne.fit_transform(x, init=1e-4 * torch.randn([600, 2], generator=torch.Generator().manual_seed(0)))
    assert torch.equal(given.y, fit.y)  # an initial embedding handed in is taken as given


def test_fit_transform_refuses_bad_arguments():
    x = torch.zeros(40, 3, device=DEV)
    for bad in ({"perplexity": 40.0}, {"max_iter": 100}, {"learning_rate": "fast"}, {"init": "pca"},
                {"init": torch.zeros(39, 2)}, {"early_exaggeration": 0.5}):
        with pytest.raises(ValueError):
            tsne.fit_transform(x, **bad)


# ---------------------------------------------------------------- the Tester
from test_gpu_evaluate import CONFIG, workspace  # noqa: E402,F401  (the demo workspace fixture)


def test_tester_tsne_embeddings_on_golden_weights(workspace, tmp_path):  # noqa: F811
    """24 train + 12 test heads through the golden encoder, no classifiers:
    the file has the documented keys, train rows first."""
    import types

    from craniofacialsd_vae_amd import manager as M
    d, cfg = workspace
    cfg = {k: v for k, v in cfg.items() if k != "classifier"}
    man = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"], use_graph=False)
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    m = recipe.load_meshes()
    rs = np.random.RandomState(8)
    heads = np.stack([m["verts"][i % 12] + rs.normal(0, 0.002, m["verts"][0].shape) for i in range(36)])
    heads = torch.from_numpy(((heads - m["norm_mean"]) / m["norm_std"]).astype(np.float32)).to(DEV)
    labels = [("nacm"[i % 4], i % 3 == 0) for i in range(36)]
    sets = [types.SimpleNamespace(meshes=heads[s], labels=labels[s]) for s in (slice(0, 24), slice(24, 36))]
    stats = {k: torch.zeros(75) for k in ("means", "stds", "mins", "maxs")}
    t = evaluation.Tester(man, None, sets[0], sets[1], str(tmp_path), cfg, latent_stats=stats)
    assert not t.has_classifiers
    path = t.tsne_embeddings(perplexity=5.0, generator=torch.Generator().manual_seed(3))
    emb = np.load(path)
    assert os.path.basename(path) == "tsne_embeddings.npz"
    assert sorted(emb.files) == sorted(["x1", "x2", "class", "is_test", "augmented", "kl_divergence", "n_iter",
                                        "perplexity"])
    assert emb["x1"].shape == emb["x2"].shape == emb["class"].shape == emb["is_test"].shape == emb["augmented"].shape == (36,)
    assert emb["class"].tolist() == [lab[0] for lab in labels] and emb["augmented"].tolist() == [lab[1] for lab in labels]
    assert emb["is_test"].tolist() == [False] * 24 + [True] * 12
    assert np.isfinite(emb["x1"]).all() and np.isfinite(emb["x2"]).all() and np.ptp(emb["x1"]) > 0
    assert np.isfinite(emb["kl_divergence"]) and 0 < emb["n_iter"] <= 999 and emb["perplexity"] == 5.0
    with pytest.raises(NotImplementedError):
        t.embeddings(mode="tsne")


def test_evaluate_only_tsne(workspace):  # noqa: F811
    """One epoch without a classifier section, then ``evaluate.py --only
    tsne``: the step runs on a run that has no classifier files."""
    import yaml

    from craniofacialsd_vae_amd import train as T
    d, cfg = workspace
    cfg = {k: v for k, v in cfg.items() if k != "classifier"}
    cfg["optimization"] = dict(cfg["optimization"], epochs=1)
    with open(d / "config_tsne.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    T.main(["--config", str(d / "config_tsne.yaml"), "--id", "ts", "--output_path", str(d / "runs_tsne")])
    tester = evaluation.evaluate_main(["--id", "ts", "--output_path", str(d / "runs_tsne"), "--seed", "5", "--only", "tsne"])
    assert not tester.has_classifiers
    emb = np.load(d / "runs_tsne" / "outputs" / "ts" / "tsne_embeddings.npz")
    n_all = tester._train_set.meshes.shape[0] + tester._test_set.meshes.shape[0]
    assert emb["x1"].shape == emb["class"].shape == (n_all,) and emb["is_test"].sum() == tester._test_set.meshes.shape[0]
    assert np.isfinite(emb["x1"]).all() and np.isfinite(emb["x2"]).all() and emb["perplexity"] == 30.0
