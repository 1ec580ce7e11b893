"""Float64 restatement of scikit-learn 1.7.2's t-SNE (``method='barnes_hut'``,
``angle=0``, two components) for the t-SNE tests: NumPy only, dense where
scikit-learn is sparse.  ``tests/golden/make_tsne.py`` pins it on
scikit-learn's own functions; the GPU tests compare the kernels with it.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def knn(z, k):
    """Top ``k`` other rows per row by ``(d2, index)``: ``(idx [n, k] int64, d2
    [n, k] float64)``; distances in difference form, float64 (exact for
    small-integer coordinates, int64 input included)."""
    z = np.asarray(z)
    z = z.astype(np.int64) if z.dtype.kind in "iu" else z.astype(np.float64)
    n = z.shape[0]
    d2 = np.zeros((n, n), z.dtype)
    for c in range(z.shape[1]):  # one [n, n] slab at a time
        t = z[:, c, None] - z[None, :, c]
        d2 += t * t
    idx = np.empty((n, k), np.int64)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        order = np.lexsort((others, d2[i, others]))[:k]
        idx[i] = others[order]
    return idx, np.take_along_axis(d2, idx, axis=1).astype(np.float64)


def perplexity_search(d2, perplexity):
    """``_binary_search_perplexity`` (``sklearn/manifold/_utils.pyx``): ``d2``
    ``[n, k]`` (used at the precision given) -> ``(p_cond [n, k] float64, beta
    [n])``, ``beta`` the last precision evaluated (the one ``p_cond`` holds)."""
    d2 = np.asarray(d2).astype(np.float64)
    want = np.log(np.float64(np.float32(perplexity)))
    tiny, tol = np.float64(np.float32(1e-8)), np.float64(np.float32(1e-5))
    p_cond, betas = np.zeros_like(d2), np.zeros(d2.shape[0])
    for i, row in enumerate(d2):
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(100):
            with np.errstate(under="ignore"):
                e = np.exp(-row * beta)
            s = e.sum()
            if s == 0.0:
                s = tiny
            p = e / s
            betas[i], p_cond[i] = beta, p
            diff = np.log(s) + beta * (row * p).sum() - want
            if abs(diff) <= tol:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    return p_cond, betas


def entropy(p):
    """Shannon entropy (nats) of every row of ``p``; ``0 log 0 = 0``."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)


def symmetrize(idx, p_cond):
    """``_joint_probabilities_nn``'s ``P = (P_cond + P_cond^T) / sum`` as a
    dense float64 ``[n, n]``."""
    n = idx.shape[0]
    dense = np.zeros((n, n))
    dense[np.arange(n)[:, None], np.asarray(idx, np.int64)] = np.asarray(p_cond, np.float64)
    dense = dense + dense.T
    return dense / max(dense.sum(), EPS)


def to_csr(dense):
    """``(row_ptr, col, val)`` of the non-zero entries, columns ascending."""
    rows, cols = np.nonzero(dense)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=dense.shape[0]))])
    return row_ptr.astype(np.int64), cols.astype(np.int64), dense[rows, cols]


def from_csr(row_ptr, col, val, n=None):
    n = len(row_ptr) - 1 if n is None else n
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(row_ptr)), col] = val
    return dense


def kl_and_grad(p, y, exaggeration=1.0):
    """``_kl_divergence_bh(angle=0, compute_error=True)`` with exact float64
    sums: ``p`` dense ``[n, n]``, ``y`` ``[n, 2]`` -> ``(KL, grad [n, 2])``."""
    p = np.asarray(p, np.float64) * exaggeration
    y = np.asarray(y).astype(np.float64)
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    z = max(q.sum(), EPS)
    attr = ((p * q)[:, :, None] * diff).sum(1)
    rep = ((q * q)[:, :, None] * diff).sum(1)
    nz = p > 0
    kl = (p[nz] * np.log(p[nz] / (q[nz] / z))).sum()
    return kl, 4.0 * (attr - rep / z)


def update_rule(y, update, gains, grad, momentum, learning_rate):
    """``_gradient_descent``'s rule in float64: returns ``(y, update, gains,
    |gains * grad|)`` after one iteration (the inputs are left alone)."""
    y, update, gains, grad = (np.asarray(a).astype(np.float64) for a in (y, update, gains, grad))
    inc = update * grad < 0.0
    gains = np.clip(np.where(inc, gains + 0.2, gains * 0.8), 0.01, np.inf)
    step = gains * grad
    update = momentum * update - learning_rate * step
    return y + update, update, gains, np.linalg.norm(step)


def fit(p, y0, early_exaggeration=12.0, learning_rate=None, max_iter=1000, n_iter_without_progress=300,
        min_grad_norm=1e-7):
    """``TSNE._tsne``'s schedule with the exact float64 gradient: ``(y, KL,
    n_iter)``."""
    n = p.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate is None else learning_rate
    y, error, it = np.asarray(y0, np.float64).copy(), np.finfo(float).max, -1
    for last, momentum, window, exag in ((250, 0.5, 250, early_exaggeration),
                                         (max_iter, 0.8, n_iter_without_progress, 1.0)):
        first = it + 1
        update, gains = np.zeros((n, 2)), np.ones((n, 2))  # every _gradient_descent call starts them afresh
        best_error, best_iter = np.finfo(float).max, first
        for it in range(first, last):
            kl, grad = kl_and_grad(p, y, exag)
            y, update, gains, norm = update_rule(y, update, gains, grad, momentum, lr)
            if (it + 1) % 50 == 0 or it == last - 1:
                error = kl
            if (it + 1) % 50 == 0:
                if error < best_error:
                    best_error, best_iter = error, it
                elif it - best_iter > window:
                    break
                if norm <= min_grad_norm:
                    break
    return y, error, it


def clusters(seed=7, per=150, d=33, n_clusters=4):
    """The whole-fit input: ``n_clusters`` Gaussian clusters of ``per`` points,
    centres ``4 * randn``, unit spread -> ``(x [n, d] float32, label [n])``."""
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.randn(n_clusters, d)
    x = np.concatenate([c + rs.randn(per, d) for c in centres]).astype(np.float32)
    return x, np.repeat(np.arange(n_clusters), per)
