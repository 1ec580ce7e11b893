"""t-SNE of a set of latents on the device: the second branch of the
reference's ``plot_embeddings`` (``test.py:1177-1180``:
``sklearn.manifold.TSNE(n_components=2, init='random')``).

The algorithm is scikit-learn 1.7.2's ``TSNE`` with ``method='barnes_hut'`` at
``angle = 0``: kNN-sparse input affinities (``_joint_probabilities_nn``), the
exact N^2 repulsive term in the place of the Barnes-Hut tree
(``_kl_divergence_bh``), two output dimensions, and ``TSNE._tsne``'s schedule
around ``_gradient_descent``.  The kernels are ``csrc/tsne.hip``
(``ops.knn_rows``, ``ops.tsne_affinities``, ``ops.tsne_step``); nothing here
imports scikit-learn.  Not reproduced: ``angle > 0``, ``n_components != 2``,
other metrics, PCA initialisation.
"""
import collections

import torch

from . import ops

EXPLORATION_ITER = 250  # TSNE._EXPLORATION_MAX_ITER: iterations with early exaggeration, momentum 0.5
N_ITER_CHECK = 50       # TSNE._N_ITER_CHECK: iterations between two progress checks
_FLOAT_MAX = float(torch.finfo(torch.float64).max)

TsneResult = collections.namedtuple("TsneResult", "y kl_divergence n_iter")


def _descend(y, csr, workspace, it, max_iter, momentum, learning_rate, exaggeration, n_iter_without_progress,
             min_grad_norm):
    """``_gradient_descent`` (``sklearn/manifold/_t_sne.py``) from iteration
    ``it``: ``update`` and ``gains`` start afresh, the error and the gradient
    norm are evaluated every ``N_ITER_CHECK`` iterations and on the last one,
    with the reference's two break rules.  The iterations between two checks
    are enqueued without synchronisation; a check reads two floats back.
    Returns ``(error, last iteration)``."""
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    grad, result = torch.empty_like(y), torch.empty(2, dtype=torch.float32, device=y.device)
    error = best_error = _FLOAT_MAX
    best_iter = i = it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        want = check or i == max_iter - 1
        ops.tsne_step(y, update, gains, csr, momentum, learning_rate, exaggeration=exaggeration, want_error=want,
                      workspace=workspace, grad=grad, result=result)
        if want:
            error, grad_norm = result.tolist()
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return error, i


def fit_transform(z, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                  n_iter_without_progress=300, min_grad_norm=1e-7, init="random", generator=None):
    """``TSNE(n_components=2, method='barnes_hut', angle=0).fit_transform(z)``
    for ``z`` ``[n, d]`` float32 on the device.  ``TSNE._tsne``'s schedule:
    ``EXPLORATION_ITER`` iterations at momentum 0.5 on ``P * early_exaggeration``
    (that stage's no-progress window is its own length), then momentum 0.8 on
    ``P`` up to ``max_iter``; ``learning_rate="auto"`` is ``max(n /
    early_exaggeration / 4, 50)``.  ``init="random"`` draws ``1e-4 * randn`` on
    the CPU from ``generator`` (a ``torch.Generator``; the default one if
    ``None``); a tensor ``[n, 2]`` is taken as given.  Returns ``TsneResult(y
    [n, 2] on the device, kl_divergence, n_iter)``, the last two as
    ``TSNE.kl_divergence_`` and ``TSNE.n_iter_``.  The same input and seed give
    the same bits."""
    if not torch.is_tensor(z) or not z.is_cuda:
        raise ValueError("z must be a device tensor")
    if z.dim() != 2:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [n, d]")
    n = int(z.shape[0])
    max_iter = int(max_iter)
    if max_iter < EXPLORATION_ITER:
        raise ValueError(f"max_iter {max_iter} < {EXPLORATION_ITER}")
    if not float(early_exaggeration) >= 1.0:
        raise ValueError(f"early_exaggeration {early_exaggeration} < 1")
    csr = ops.tsne_joint_probabilities(z.detach().to(torch.float32).contiguous(), perplexity)
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate {learning_rate!r}: a number or 'auto'")
        learning_rate = max(n / float(early_exaggeration) / 4.0, 50.0)
    if torch.is_tensor(init):
        if tuple(init.shape) != (n, 2):
            raise ValueError(f"init: shape {tuple(init.shape)}, expected [{n}, 2]")
        y = init.detach().to(z.device, torch.float32).clone().contiguous()
    elif init == "random":
        y = (1e-4 * torch.randn([n, 2], generator=generator)).to(z.device, torch.float32)
    else:
        raise ValueError(f"init {init!r}: 'random' or a tensor [n, 2]")
    workspace = ops.tsne_workspace(n, 0, z.device)
    error, it = _descend(y, csr, workspace, 0, EXPLORATION_ITER, 0.5, learning_rate, float(early_exaggeration),
                         EXPLORATION_ITER, min_grad_norm)
    if max_iter > EXPLORATION_ITER:
        error, it = _descend(y, csr, workspace, it + 1, max_iter, 0.8, learning_rate, 1.0,
                             int(n_iter_without_progress), min_grad_norm)
    return TsneResult(y, float(error), int(it))
