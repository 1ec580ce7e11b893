"""The classifier stage after the VAE (``ModelManager.train_and_validate_classifiers``,
``model_manager.py:403-573``): the MLP classifier trained on the training
latents, LDA and QDA on the full latent, and one LDA / QDA per latent region.

The hot paths are libcfsd kernels (``csrc/classify.hip``): per-class
statistics and discriminant scores for LDA / QDA, the MLP's forward and its
fused train step (two launches per step, one ctypes call per epoch).  The
``d x d`` eigendecompositions that turn statistics into a classifier run on the
host in float64 (``finish_qda`` / ``finish_lda``; d <= 128).

The reference fits scikit-learn objects and pickles them.  Here the
classifiers are restated (formulas below, checked against scikit-learn 1.7.2 by
``tests/golden/make_classify.py``) and saved as dictionaries of tensors: no
pickle is executed on load.  ``LinearSVC`` is not provided.
"""
import math
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import ops

# Eigenvalues of a covariance below this fraction of its largest are raised to
# it: the statistics are fp32, so nothing below ~1e-7 of the largest is
# resolved.  Well-conditioned classes (what scikit-learn handles without its
# "variables are collinear" warning) never reach the floor.
EIG_FLOOR = 1e-7

MAIN_MODEL_TYPES = ("mlp", "lda", "qda", "none")


# ---------------------------------------------------------------- configuration
def classifier_params(config, *, end2end=False):
    """The validated ``classifier:`` section of a configuration, or None when
    there is none (then nothing of this module is constructed).  ``svm``
    (liblinear's coordinate descent has no place on this path) is refused.
    ``mlp_training_type: end2end`` (the classifier's loss inside the VAE step)
    is accepted only from a caller that trains it there (``end2end=True``:
    ``manager.ModelManager``); it then needs a finite ``mlp_loss_weight`` and
    an ``optimization.batch_size`` the head kernel takes (<= 16)."""
    p = config.get("classifier")
    if p is None:
        return None
    main = str(p.get("main_model_type", "qda"))
    if main == "svm":
        raise ValueError("classifier.main_model_type: svm is not supported (LinearSVC is not part of this "
                         "package); use mlp, lda or qda")
    if main not in MAIN_MODEL_TYPES:
        raise ValueError(f"classifier.main_model_type: {main!r}, expected one of {MAIN_MODEL_TYPES}")
    if str(p.get("mlp_training_type", "after")) == "end2end" and end2end:
        w = p.get("mlp_loss_weight")
        try:  # (PyYAML reads 1e-3 as a string: numbers are taken as the other weights are, through float())
            ok = not isinstance(w, bool) and math.isfinite(float(w))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"classifier.mlp_loss_weight: {w!r}, a finite number is required with "
                             "mlp_training_type: end2end")
        bs = int(config.get("optimization", {}).get("batch_size", 1))
        if bs > ops.MLP_MAX_BS:
            raise ValueError(f"optimization.batch_size {bs}: mlp_training_type: end2end takes at most "
                             f"{ops.MLP_MAX_BS}")
        return dict(p)
    if str(p.get("mlp_training_type", "after")) == "end2end":
        raise NotImplementedError("classifier.mlp_training_type: end2end (the classifier loss inside the VAE "
                                  "step) is not implemented by this caller; use 'after'")
    if str(p.get("mlp_training_type", "after")) != "after":
        raise ValueError(f"classifier.mlp_training_type: {p.get('mlp_training_type')!r}, expected 'after'")
    return dict(p)


def class_order_and_weights(counts, classes=None):
    """``set_class_conversions_and_weights`` (``model_manager.py:548-555`` over
    ``compute_classes_and_weights``, ``data_loading.py:152-161``): ``counts``
    maps a class letter to its number of training meshes ('b' already folded
    into 'n' by ``data.labels_of``).  Classes are ordered by letter; the
    weights are ``1 / count`` normalised to sum 1.  ``classes`` (optional)
    names every class of the data set: one without a training mesh keeps its
    place in the order and gets weight 0 (the reference cannot represent it).
    Returns ``(class2idx, weights float32 [C])``."""
    letters = sorted(counts) if classes is None else sorted(classes)
    if not counts or set(counts) - set(letters) or min(counts.values()) < 1:
        raise ValueError(f"class counts {counts} for the classes {letters}: every counted class needs at least "
                         "one mesh and must be one of the classes")
    w = np.array([1.0 / counts[k] if k in counts else 0.0 for k in letters], np.float64)
    return {k: i for i, k in enumerate(letters)}, (w / w.sum()).astype(np.float32)


def count_labels(labels):
    """Letter -> count of a label list (``ResidentData.labels`` entries or letters)."""
    out = {}
    for lab in labels:
        y = lab[0] if isinstance(lab, (tuple, list)) else lab
        out[y] = out.get(y, 0) + 1
    return out


# ---------------------------------------------------------------- MLP
class MLPClassifier(nn.Module):
    """The reference's ``MLPClassifier`` (``model.py:191-203``): ``Linear`` +
    ``ReLU`` per layer, the last included, with the same ``state_dict`` keys
    (``model.0.weight``, ``model.0.bias``, ``model.2.weight``, ...).  The
    parameters are views of ONE flat device buffer (``flat``) with the Adam
    moments next to it; :meth:`forward` and :meth:`run_epoch` run libcfsd
    kernels on it (no autograd)."""

    def __init__(self, in_features, hidden_features, out_classes, device="cuda", seed=0, lr=1e-4, weight_decay=0.0):
        super().__init__()
        self.dims = [int(in_features)] + [int(h) for h in hidden_features] + [int(out_classes)]
        ops.mlp_dims(self.dims)
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        device = torch.device(device)
        n = ops.mlp_param_count(self.dims)
        g = torch.Generator().manual_seed(int(seed))
        flat = torch.empty(n, dtype=torch.float32)
        layers, off = [], 0
        for i in range(1, len(self.dims)):
            n_in, n_out = self.dims[i - 1], self.dims[i]
            # nn.Linear.reset_parameters: kaiming_uniform(a = sqrt(5)) and the
            # bias bound are both U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
            bound = 1.0 / math.sqrt(n_in)
            cnt = n_out * n_in + n_out
            flat[off:off + cnt] = (torch.rand(cnt, generator=g) * 2 - 1) * bound
            off += cnt
            layers += [nn.Linear(n_in, n_out), nn.ReLU()]
        self.model = nn.Sequential(*layers)
        self.flat = flat.to(device)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self._acc = torch.zeros(3, dtype=torch.float32, device=device)
        self._workspace = None
        off = 0
        for i in range(1, len(self.dims)):
            n_in, n_out = self.dims[i - 1], self.dims[i]
            lin = self.model[2 * (i - 1)]
            lin.weight = nn.Parameter(self.flat[off:off + n_out * n_in].view(n_out, n_in), requires_grad=False)
            off += n_out * n_in
            lin.bias = nn.Parameter(self.flat[off:off + n_out], requires_grad=False)
            off += n_out

    def _rows(self, z):
        return z.detach().to(self.flat.device, torch.float32).reshape(-1, self.dims[0]).contiguous()

    @torch.no_grad()
    def forward(self, z):
        """``(out, out_label)`` as the reference (``model.py:200-203``): the
        post-ReLU logits ``[n, C]`` and their arg max (int64)."""
        out, pred = ops.mlp_forward(self._rows(z), self.flat, self.dims)
        return out, pred.long()

    @torch.no_grad()
    def run_epoch(self, z, labels, class_weights, bs, train=True, dw_out=None):
        """``mlp_classifier_epoch`` (``model_manager.py:428-446``) over the
        batches of ``bs`` consecutive rows of ``z`` ``[N, in]`` / ``labels``
        ``[N]`` (int32, device), a ragged tail left out: one library call.
        Returns ``(mean loss, mean accuracy in percent)`` over the batches."""
        z = self._rows(z)
        n_steps = z.shape[0] // int(bs)
        if n_steps < 1:
            raise ValueError(f"{z.shape[0]} rows hold no batch of {bs}")
        if train and self._workspace is None:
            self._workspace = torch.empty(ops.mlp_workspace(self.dims, ops.MLP_MAX_BS) // 4 + 1,
                                          dtype=torch.float32, device=self.flat.device)
        self._acc.zero_()
        ops.mlp_train_steps(z, labels, class_weights, self.flat, self.exp_avg, self.exp_avg_sq, self.step, self._acc,
                            self.dims, int(bs), n_steps, train=train, lr=self.lr, weight_decay=self.weight_decay,
                            workspace=self._workspace, dw_out=dw_out)
        a = self._acc.cpu().numpy().astype(np.float64)
        return a[0] / a[2], a[1] / a[2]


# ---------------------------------------------------------------- LDA / QDA, host side
def _whitening(cov, what):
    """``V / sqrt(w)`` and ``w`` of the eigendecomposition ``V diag(w) V^T``."""
    w, v = np.linalg.eigh(cov)
    floor = EIG_FLOOR * max(float(w[-1]), np.finfo(np.float64).tiny)
    if w[0] < floor:
        warnings.warn(f"{what}: covariance is not full rank (smallest / largest eigenvalue "
                      f"{w[0] / max(w[-1], np.finfo(np.float64).tiny):.1e}); small eigenvalues are raised to "
                      f"{EIG_FLOOR:g} of the largest")
        w = np.maximum(w, floor)
    return v / np.sqrt(w), w


def _check_counts(count):
    count = np.asarray(count, np.int64)
    if count.min() < 2:
        raise ValueError(f"class sizes {count.tolist()}: every class needs at least 2 rows")
    return count, int(count.sum())


def finish_qda(count, mean, scatter):
    """QDA from per-class statistics (float64): per class the covariance
    ``S_c / (n_c - 1) = V diag(w) V^T``, ``whiten_c = V / sqrt(w)`` and
    ``offset_c = -0.5 sum(log w) + log prior_c`` (scikit-learn's
    ``QuadraticDiscriminantAnalysis`` decision function is ``-0.5 |(z -
    mean_c) whiten_c|^2 + offset_c``); priors ``n_c / n``."""
    count, n = _check_counts(count)
    mean, scatter = np.asarray(mean, np.float64), np.asarray(scatter, np.float64)
    priors = count / n
    cov = scatter / (count - 1)[:, None, None]
    whiten, offset = np.empty_like(cov), np.empty(len(count))
    for c in range(len(count)):
        whiten[c], w = _whitening(cov[c], f"QDA class {c}")
        offset[c] = -0.5 * np.log(w).sum() + np.log(priors[c])
    return {"means": mean, "covariance": cov, "priors": priors, "count": count, "whiten": whiten, "offset": offset}


def finish_lda(count, mean, scatter, n_components=2):
    """LDA from per-class statistics (float64): the pooled ``S_w = sum_c S_c /
    (n - C)`` gives the shared whitening, ``offset_c = log prior_c``;
    ``covariance`` is scikit-learn's ``sum_c prior_c S_c / n_c``; the
    ``n_components`` projection is ``whiten . Vt[:k]^T`` applied to ``z -
    xbar``, ``xbar = sum_c prior_c mean_c``, ``Vt`` from the SVD of
    ``sqrt(n_c / (C - 1)) (mean_c - xbar) . whiten``."""
    count, n = _check_counts(count)
    mean, scatter = np.asarray(mean, np.float64), np.asarray(scatter, np.float64)
    n_cls = len(count)
    if n <= n_cls:
        raise ValueError(f"{n} rows in {n_cls} classes: LDA needs more rows than classes")
    priors = count / n
    whiten, _ = _whitening(scatter.sum(0) / (n - n_cls), "LDA")
    xbar = priors @ mean
    m = np.sqrt(count / max(n_cls - 1, 1))[:, None] * (mean - xbar) @ whiten
    vt = np.linalg.svd(m, full_matrices=False)[2]
    k = max(min(n_components, n_cls - 1, mean.shape[1]), 1)
    return {"means": mean, "covariance": (priors[:, None, None] * scatter / count[:, None, None]).sum(0),
            "priors": priors, "count": count, "whiten": whiten[None], "offset": np.log(priors), "xbar": xbar,
            "projection": whiten @ vt[:k].T}


class _Discriminant:
    """Common part of :class:`LinearDiscriminant` / :class:`QuadraticDiscriminant`:
    statistics and scores on the device, the fit finished on the host."""
    _finish = None
    _tensor_keys = ("means", "covariance", "priors", "count", "whiten", "offset", "classes")

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.cols = None
        self._fit = None

    # -- fitting
    def fit(self, z, y, cols=None, n_classes=None):
        """``z`` ``[n, ld]`` device latents, ``y`` ``[n]`` class indices,
        ``cols = (col0, d)`` the column window (default: every column).  A
        class with fewer than 2 rows raises ``ValueError``."""
        z = z.detach().to(self.device, torch.float32).contiguous()
        y = torch.as_tensor(y).to(self.device, torch.int32).contiguous()
        if n_classes is None:
            n_classes = int(y.max().item()) + 1
        count, mean, scatter = ops.class_stats(z, y, n_classes, cols)
        count = count.cpu().numpy()
        keep = np.nonzero(count > 0)[0]  # scikit-learn's classes_: the labels that occur
        fit = type(self)._finish(count[keep], mean.cpu().double().numpy()[keep], scatter.cpu().double().numpy()[keep])
        fit["classes"] = keep.astype(np.int64)
        self._install(fit, cols)
        return self

    def _install(self, fit, cols):
        self._fit = {k: np.asarray(v) for k, v in fit.items()}
        self.cols = None if cols is None else (int(cols[0]), int(cols[1]))
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device)  # noqa: E731
        self._mean, self._whiten, self._offset = f32(fit["means"]), f32(fit["whiten"]), f32(fit["offset"])
        self._classes = torch.as_tensor(np.asarray(fit["classes"], np.int64)).to(self.device)

    def _fitted(self):
        if self._fit is None:
            raise RuntimeError(f"{type(self).__name__} is not fitted")
        return self._fit

    # -- scikit-learn's attributes
    means_ = property(lambda self: self._fitted()["means"])
    covariance_ = property(lambda self: self._fitted()["covariance"])
    priors_ = property(lambda self: self._fitted()["priors"])
    classes_ = property(lambda self: self._fitted()["classes"])

    def class_position(self, class_idx):
        """Column of class ``class_idx`` in the per-class outputs (the classes
        that occurred in the fit, ascending)."""
        pos = np.nonzero(self.classes_ == int(class_idx))[0]
        if not len(pos):
            raise KeyError(f"class {class_idx} did not occur in the fit (classes {self.classes_.tolist()})")
        return int(pos[0])

    # -- scoring (device tensors)
    def _scores(self, z, **want):
        self._fitted()
        z = z.detach().to(self.device, torch.float32)
        z = (z.unsqueeze(0) if z.dim() == 1 else z).contiguous()
        return ops.discriminant_scores(z, self._mean, self._whiten, self._offset, self.cols, **want)

    def decision_function(self, z):
        """``[n, len(classes_)]`` class scores ``-0.5 maha2 + offset`` (for
        LDA equal to scikit-learn's up to a constant per row)."""
        return self._scores(z, want_pred=False)["scores"]

    def predict(self, z):
        return self._classes[self._scores(z, want_scores=False)["pred"].long()]

    def predict_log_proba(self, z):
        return torch.log_softmax(self.decision_function(z), dim=1)

    def mahalanobis2(self, z):
        """``[n, len(classes_)]`` squared Mahalanobis distances to every class."""
        return self._scores(z, want_maha2=True, want_scores=False, want_pred=False)["maha2"]

    def score(self, z, y):
        """Mean accuracy (a fraction, as scikit-learn's ``score``)."""
        y = torch.as_tensor(y).to(self.device).long()
        return float((self.predict(z) == y).float().mean().item())

    # -- persistence (tensors only)
    def state_dict(self):
        f = self._fitted()
        sd = {k: torch.from_numpy(np.ascontiguousarray(f[k])) for k in self._tensor_keys}
        sd["cols"] = torch.tensor(self.cols if self.cols is not None else (-1, -1), dtype=torch.int64)
        return sd

    def load_state_dict(self, sd):
        missing = [k for k in self._tensor_keys + ("cols",) if k not in sd]
        if missing:
            raise KeyError(f"{type(self).__name__} state lacks {missing}")
        cols = tuple(int(v) for v in sd["cols"].tolist())
        self._install({k: sd[k].cpu().numpy() for k in self._tensor_keys}, None if cols[0] < 0 else cols)
        return self


class QuadraticDiscriminant(_Discriminant):
    """scikit-learn's ``QuadraticDiscriminantAnalysis(store_covariance=True)``
    restated (:func:`finish_qda`)."""
    _finish = staticmethod(finish_qda)

    def sample(self, class_idx, n_samples=1, generator=None):
        """``n_samples`` draws of class ``class_idx``'s Gaussian (the
        reference's ``np.random.multivariate_normal``): mean + Cholesky factor
        times normal draws, on the device."""
        pos = self.class_position(class_idx)
        cov = self.covariance_[pos]
        try:
            factor = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:  # semi-definite (fewer rows than dimensions): any A with A A^T = cov serves
            w, v = np.linalg.eigh(cov)
            factor = v * np.sqrt(np.maximum(w, 0.0))
        factor = torch.as_tensor(factor, dtype=torch.float32).to(self.device)
        eps = torch.randn((int(n_samples), factor.shape[0]), generator=generator, device=self.device)
        return self._mean[pos] + eps @ factor.T


class LinearDiscriminant(_Discriminant):
    """scikit-learn's ``LinearDiscriminantAnalysis(n_components=2,
    store_covariance=True)`` restated (:func:`finish_lda`)."""
    _finish = staticmethod(finish_lda)
    _tensor_keys = _Discriminant._tensor_keys + ("xbar", "projection")

    def _install(self, fit, cols):
        super()._install(fit, cols)
        self._xbar = torch.as_tensor(fit["xbar"], dtype=torch.float32).to(self.device)
        self._projection = torch.as_tensor(np.ascontiguousarray(fit["projection"]), dtype=torch.float32).to(self.device)

    def transform(self, z):
        """The discriminant components of ``z`` (``[n, 2]``; each component
        is defined up to its sign)."""
        self._fitted()
        z = z.detach().to(self.device, torch.float32)
        z = z.unsqueeze(0) if z.dim() == 1 else z
        if self.cols is not None:
            z = z[:, self.cols[0]:self.cols[0] + self.cols[1]]
        return (z - self._xbar) @ self._projection


# ---------------------------------------------------------------- ModelManager part
def _save(obj, path):
    torch.save(obj, path)
    return path


class ClassifierStage:
    """What ``ModelManager`` gains from a ``classifier:`` section.  Mixed into
    ``manager.ModelManager``; without the section ``_init_classifiers`` leaves
    ``_classifier_params = None`` and constructs nothing."""

    def _init_classifiers(self, configurations, seed=0, end2end=False):
        """``end2end``: the caller can train the MLP inside the VAE step."""
        self._classifier_params = classifier_params(configurations, end2end=end2end)
        self._class2idx_dict, self._class_weights = None, None
        self._mlp_end2end = False
        if self._classifier_params is None:
            return
        self._mlp_end2end = str(self._classifier_params.get("mlp_training_type", "after")) == "end2end"
        from .data import labels_of
        cp = self._classifier_params
        names = [n for n in os.listdir(configurations["data"]["dataset_path"]) if n.endswith(".obj")]
        letters = sorted({labels_of(n)[0] for n in names})  # model_manager.py:107-108, 'b' folded into 'n'
        self._class2idx_dict = {k: i for i, k in enumerate(letters)}
        self.classifier_mlp = MLPClassifier(
            self._model_params["latent_size"], cp["mlp_hidden_features"], len(letters), device=self.device,
            seed=seed, lr=float(cp["mlp_lr"]), weight_decay=float(self._optimization_params["weight_decay"]))
        self.lda = LinearDiscriminant(self.device)
        self.qda = QuadraticDiscriminant(self.device)
        self.region_ldas, self.region_qdas = None, None
        if self._w_latent_cons_loss > 0:
            self.region_ldas = {k: LinearDiscriminant(self.device) for k in self.latent_regions}
            self.region_qdas = {k: QuadraticDiscriminant(self.device) for k in self.latent_regions}

    def _need_classifiers(self):
        if getattr(self, "_classifier_params", None) is None:
            raise RuntimeError("the configuration has no classifier: section")

    # -- classes
    def set_class_conversions_and_weights(self, counts):
        """``counts``: class letter -> number of training meshes.  The classes
        are those of the data set folder (as the reference counts them at
        construction); one without a training mesh gets weight 0."""
        self._need_classifiers()
        c2i, w = class_order_and_weights(counts, sorted(set(self._class2idx_dict) | set(counts)))
        if len(c2i) != self.classifier_mlp.dims[-1]:
            raise ValueError(f"{len(c2i)} classes {sorted(c2i)}, the MLP classifier has "
                             f"{self.classifier_mlp.dims[-1]} outputs")
        self._class2idx_dict = c2i
        self._class_weights = torch.from_numpy(w).to(self.device)

    def set_class_conversions(self, class2idx_dict):
        self._class2idx_dict = dict(class2idx_dict)

    @property
    def class2idx_dict(self):
        return dict(self._class2idx_dict)

    def class2idx(self, data_class):
        if isinstance(data_class, (list, tuple, np.ndarray)):
            return [self._class2idx_dict[d] for d in data_class]
        return self._class2idx_dict[data_class]

    def idx2class(self, idx):
        inv = {v: k for k, v in self._class2idx_dict.items()}
        if torch.is_tensor(idx):
            idx = idx.cpu().numpy()
        if isinstance(idx, (list, tuple, np.ndarray)):
            return [inv[int(i)] for i in idx]
        return inv[int(idx)]

    # -- training
    def _classifier_rows(self, data):
        """Eval-mode latents and class indices of a resident set, in file
        order, rows ``[0, (N // bs) bs)``: the rows one drop_last epoch visits."""
        n = (data.meshes.shape[0] // self.bs) * self.bs
        z = self.encode(data.meshes[:n]).contiguous()
        y = torch.tensor(self.class2idx([lab[0] for lab in data.labels[:n]]), dtype=torch.int32).to(self.device)
        return z, y

    def train_and_validate_classifiers(self, train_set, val_set, writer, checkpoint_dir):
        """``model_manager.py:448-504`` without the SVM: ``mlp_epochs`` epochs
        of the MLP in batches of ``batch_size`` consecutive latents (scalars
        ``{train,validation}/class_{loss,acc}`` per epoch; none with
        ``mlp_training_type: end2end``, whose MLP was trained inside the VAE
        step and is only validated here, ``:457``), LDA and QDA on the
        full latent, one LDA / QDA per latent region when the latent
        consistency weight is above 0; the five files are written into
        ``checkpoint_dir``.  Returns the validation accuracies in percent
        (None without a validation set)."""
        self._need_classifiers()
        cp = self._classifier_params
        if self._class_weights is None:
            self.set_class_conversions_and_weights(count_labels(train_set.labels))
        z, y = self._classifier_rows(train_set)
        zv, yv = self._classifier_rows(val_set) if val_set is not None else (None, None)
        mlp, w = self.classifier_mlp, self._class_weights
        for epoch in range(0 if self._mlp_end2end else int(cp["mlp_epochs"])):
            tr_loss, tr_acc = mlp.run_epoch(z, y, w, self.bs, train=True)
            if writer is not None:
                writer.add_scalar("train/class_loss", tr_loss, epoch + 1)
                writer.add_scalar("train/class_acc", tr_acc, epoch + 1)
            if zv is not None:
                va_loss, va_acc = mlp.run_epoch(zv, yv, w, self.bs, train=False)
                if writer is not None:
                    writer.add_scalar("validation/class_loss", va_loss, epoch + 1)
                    writer.add_scalar("validation/class_acc", va_acc, epoch + 1)
        acc = {"mlp": None, "lda": None, "qda": None}
        if zv is not None:
            acc["mlp"] = mlp.run_epoch(zv, yv, w, self.bs, train=False)[1]
        n_cls = len(self._class2idx_dict)
        self.lda.fit(z, y, n_classes=n_cls)
        self.qda.fit(z, y, n_classes=n_cls)
        if zv is not None:
            acc["lda"] = 100.0 * self.lda.score(zv, yv)
            acc["qda"] = 100.0 * self.qda.score(zv, yv)
        if self.region_ldas is not None:
            for key, (lo, hi) in self.latent_regions.items():
                self.region_ldas[key].fit(z, y, cols=(lo, hi - lo), n_classes=n_cls)
                self.region_qdas[key].fit(z, y, cols=(lo, hi - lo), n_classes=n_cls)
        self.save_classifiers(checkpoint_dir)
        for k, v in acc.items():
            print(f"{k.upper()} validation accuracy = {v}", flush=True)
        return acc

    # -- files
    def save_classifiers(self, checkpoint_dir):
        """``mlp_classifier.pt`` in the reference's format (``{'model':
        state_dict}``); the discriminants as dictionaries of tensors (the
        reference pickles scikit-learn objects there)."""
        self._need_classifiers()
        j = lambda n: os.path.join(checkpoint_dir, n)  # noqa: E731
        _save({"model": {k: v.detach().cpu().clone() for k, v in self.classifier_mlp.state_dict().items()}},
              j("mlp_classifier.pt"))
        _save(self.lda.state_dict(), j("lda_classifier.pt"))
        _save(self.qda.state_dict(), j("qda_classifier.pt"))
        if self.region_ldas is not None:
            _save({k: m.state_dict() for k, m in self.region_ldas.items()}, j("region_ldas.pt"))
            _save({k: m.state_dict() for k, m in self.region_qdas.items()}, j("region_qdas.pt"))

    def resume_classifiers(self, checkpoint_dir):
        """Loads whatever classifier files ``checkpoint_dir`` holds
        (``weights_only=True``); returns the names loaded."""
        self._need_classifiers()
        loaded = []

        def load(name):
            path = os.path.join(checkpoint_dir, name)
            if not os.path.exists(path):
                print(f"Can't load {name}: not trained yet.")
                return None
            loaded.append(name)
            return torch.load(path, map_location="cpu", weights_only=True)

        sd = load("mlp_classifier.pt")
        if sd is not None:
            self.classifier_mlp.load_state_dict(sd["model"])
        for name, model in (("lda_classifier.pt", self.lda), ("qda_classifier.pt", self.qda)):
            sd = load(name)
            if sd is not None:
                model.load_state_dict(sd)
        if self.region_ldas is not None:
            for name, models in (("region_ldas.pt", self.region_ldas), ("region_qdas.pt", self.region_qdas)):
                sd = load(name)
                if sd is not None:
                    for k, m in models.items():
                        m.load_state_dict(sd[k])
        return loaded

    # -- use
    @torch.no_grad()
    def classify_latent(self, z, model="main"):
        """Class letters of the latents ``z`` by ``mlp | lda | qda`` (``main``:
        the configuration's ``main_model_type``)."""
        self._need_classifiers()
        if model == "main":
            model = self._classifier_params["main_model_type"]
        if model == "mlp":
            pred = self.classifier_mlp(z)[1]
        elif model == "lda":
            pred = self.lda.predict(z)
        elif model == "qda":
            pred = self.qda.predict(z)
        else:
            raise NotImplementedError(f"classifier {model!r}")
        return self.idx2class(pred)

    def lda_project_latents_in_2d(self, latents):
        self._need_classifiers()
        return self.lda.transform(latents)

    def qda_sample(self, sample_class="a", n_samples=1, generator=None):
        self._need_classifiers()
        if isinstance(sample_class, str):
            sample_class = self.class2idx(sample_class)
        return self.qda.sample(sample_class, n_samples, generator)

    def mahalanobis_dist_to_qda_distribution(self, z, distribution_class="n", region="all"):
        """Mahalanobis distance of every row of ``z`` (full latents) to the
        QDA Gaussian of ``distribution_class``, of the whole latent or of one
        latent region; a device tensor ``[n]``."""
        self._need_classifiers()
        qda = self.qda if region == "all" else self.region_qdas[region]
        return torch.sqrt(qda.mahalanobis2(z)[:, qda.class_position(self.class2idx(distribution_class))])

    def qda_gaussian(self, distribution_class="n", region="all"):
        """``(mean [d], whiten [d, d], cols)`` of the QDA Gaussian of
        ``distribution_class``, of the whole latent or of one latent region:
        the fp32 device tensors the scores are computed from and the column
        window ``(col0, d)`` they apply to (``None``: every column).  What the
        planning kernels (``ops.plan_targets``, ``ops.pair_metrics``) read."""
        self._need_classifiers()
        qda = self.qda if region == "all" else self.region_qdas[region]
        qda._fitted()
        pos = qda.class_position(self.class2idx(distribution_class))
        return qda._mean[pos].contiguous(), qda._whiten[pos].contiguous(), qda.cols
