"""Evaluation of a trained model: the reference's ``Tester`` (``test.py:35-79``,
what ``python test.py --id X`` runs) on the libcfsd path.

Latent traversals with their per-region table, random generation, the two
diversity figures, the reconstruction errors, the classifier reports and the
interpolation pictures.  The GPU work is the existing decoder
(``manager.generate``) and rasteriser (``manager.render``) plus two kernels of
``csrc/evaluate.hip``: the distance of every traversal frame to its group's
first frame (``ops.group_vertex_errors``) and the per-region mean of a
per-vertex quantity (``ops.region_means``), so a traversal's numbers never
leave the device before they are final.

What replaces the reference's output files: mp4 videos become animated PNGs
(``rendering.save_apng``; same frames, same rates), the seaborn plots of the
traversal become ``latent_exploration.json`` (the table they draw), the
embedding plots ``lda_embeddings.npz`` and ``tsne_embeddings.npz`` (the points
they scatter; the t-SNE runs on the device, ``tsne.fit_transform``), the
confusion-matrix plots ``confusion_matrices.json`` /
``region_confusion_matrices.json``.  scikit-learn's ``classification_report``
and ``confusion_matrix`` are restated here (checked against scikit-learn 1.7.2
by ``tests/golden/make_evaluate.py``).

Surgical planning (``interpolate_syndrome_to_normal``, ``classify_and_project``,
the pre- / post-operative metrics) runs on three kernels of
``csrc/planning.hip``: the crossings of a patient's path to the healthy
distribution in closed form (``ops.plan_targets``), the latent tables of the
planned procedures (``ops.plan_tables``) and the raw quantities of every pair
and region in one launch (``ops.pair_metrics``).  The figures the reference
draws its points into become JSON files of those points.  Out of scope: the
``LinearSVC`` and the plots other than the embedding figures.

The embedding figures (class-density maps, paths to normal and pre / post
arrows on them) are drawn on the device by ``figures.py`` over three kernels
of ``csrc/figures.hip``: ``embedding_figures``, ``plan_figures``,
``prepost_figures``, the step ``figures``.

Latents are decoded in chunks of exactly ``batch_size ** 2`` rows (the last
one padded), so a decoded head does not depend on how many others were asked
for in the same call.  Every method that draws random numbers takes a CPU
``torch.Generator``: the reference draws its latents on the CPU.
"""
import json
import os

import numpy as np
import torch

from . import figures, ops, precompute, rendering, tsne

N_STEPS = 10  # frames per latent variable of a traversal (test.py:144)


# ---------------------------------------------------------------- scikit-learn's reports, restated
def _labels_of(y_true, y_pred):
    return sorted(set(y_true) | set(y_pred))


def _counts(y_true, y_pred, labels):
    pos = {lab: i for i, lab in enumerate(labels)}
    cm = np.zeros((len(labels), len(labels)), np.int64)
    for t, p in zip(y_true, y_pred):
        cm[pos[t], pos[p]] += 1
    return cm


def _as_list(y):
    if torch.is_tensor(y):
        y = y.cpu().numpy()
    return [v.item() if isinstance(v, np.generic) else v for v in list(y)]


def confusion_matrix(y_true, y_pred, normalize=None):
    """``sklearn.metrics.confusion_matrix``: rows the true labels, columns the
    predicted ones, labels the sorted union of both.  ``normalize="true"``
    divides every row by its sum; a row without support becomes zeros."""
    if normalize not in (None, "true"):
        raise ValueError('normalize must be None or "true"')
    y_true, y_pred = _as_list(y_true), _as_list(y_pred)
    if len(y_true) != len(y_pred):
        raise ValueError(f"{len(y_true)} true labels, {len(y_pred)} predictions")
    cm = _counts(y_true, y_pred, _labels_of(y_true, y_pred))
    if normalize is None:
        return cm
    sums = cm.sum(axis=1, keepdims=True).astype(np.float64)
    return np.divide(cm.astype(np.float64), sums, out=np.zeros(cm.shape, np.float64), where=sums > 0)


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(num.shape, np.float64), where=den > 0)


def classification_report(y_true, y_pred):
    """``sklearn.metrics.classification_report(output_dict=True)``: per label
    (the sorted union, keys ``str(label)``) ``precision``, ``recall``,
    ``f1-score`` (``2 tp / (true + predicted)``) and ``support``; ``accuracy``;
    the ``macro avg`` and the support-weighted ``weighted avg``.  A zero
    denominator gives 0.0."""
    y_true, y_pred = _as_list(y_true), _as_list(y_pred)
    if len(y_true) != len(y_pred) or not y_true:
        raise ValueError(f"{len(y_true)} true labels, {len(y_pred)} predictions")
    labels = _labels_of(y_true, y_pred)
    cm = _counts(y_true, y_pred, labels)
    tp, true_sum, pred_sum = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    rows = {"precision": _ratio(tp, pred_sum), "recall": _ratio(tp, true_sum),
            "f1-score": _ratio(2 * tp, true_sum + pred_sum)}
    report = {str(lab): {**{k: float(v[i]) for k, v in rows.items()}, "support": int(true_sum[i])}
              for i, lab in enumerate(labels)}
    total = int(true_sum.sum())
    report["accuracy"] = float(tp.sum() / total)
    report["macro avg"] = {**{k: float(np.mean(v)) for k, v in rows.items()}, "support": total}
    report["weighted avg"] = {**{k: float(np.sum(v * true_sum) / total) for k, v in rows.items()}, "support": total}
    return report


# ---------------------------------------------------------------- latents
def vector_linspace(start, finish, steps):
    """``Tester.vector_linspace`` (``test.py:1153-1159``): ``start`` /
    ``finish`` ``[1, d]`` -> ``[steps, d]``, column ``j`` being
    ``torch.linspace(start[0, j], finish[0, j], steps)``."""
    cols = [torch.linspace(float(s), float(f), steps) for s, f in zip(start[0], finish[0])]
    return torch.stack(cols).t()


def _quantise(images):
    """:func:`rendering.to_uint8`'s rule on a device batch ``[N, 3, H, W]``."""
    return torch.floor(images.detach().to(torch.float32).clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)


def _dump(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f)
    return path


# ---------------------------------------------------------------- surgical planning, host side
PLAN_LEVELS = (3.0, 2.0, 1.0)  # the shells of the healthy distribution a path is cut at (test.py:681-684)
PLAN_STEPS = 5000              # points of the path the crossings are searched on (test.py:693)
PLAN_FIRST = 8                 # frames from the patient to the first shell (test.py:706)
PAIR_COLUMNS = ("PID", "Pre name", "Post name", "Surgery regions", "Procedure", "Syndrome")


def planning_procedures(config, latent_regions):
    """The procedures of a run: ``planning: procedures: {name: [region key,
    ...]}`` of its configuration, validated against ``latent_regions`` (the
    reference keeps its own table in ``utils.py``); without the section one
    procedure per region, named by the region's key.  Returns ``{name: [region
    keys as they are in latent_regions]}`` in the configuration's order."""
    by_name = {str(k): k for k in latent_regions}
    section = (config.get("planning") or {}).get("procedures")
    if section is None:
        return {name: [key] for name, key in by_name.items()}
    if not isinstance(section, dict) or not section:
        raise ValueError("planning.procedures: expected a mapping {procedure name: [region key, ...]}")
    out = {}
    for name, keys in section.items():
        name = str(name)
        if not name or os.sep in name or name in (".", "..", "all_attributes"):
            raise ValueError(f"planning.procedures: {name!r} cannot name a procedure (it names its folder)")
        if isinstance(keys, (str, bytes)) or not hasattr(keys, "__iter__"):
            raise ValueError(f"planning.procedures.{name}: expected a list of region keys, got {keys!r}")
        keys = [str(k) for k in keys]
        unknown = [k for k in keys if k not in by_name]
        if not keys or unknown or len(set(keys)) != len(keys):
            raise ValueError(f"planning.procedures.{name}: {keys}: expected one or more different keys of "
                             f"{sorted(by_name)}" + (f"; unknown {unknown}" if unknown else ""))
        out[name] = [by_name[k] for k in keys]
    return out


def read_pairs_table(path):
    """The table of ``evaluate_all_pre_post_pairs`` as a pandas frame: a
    ``.csv`` (``read_csv``) or a spreadsheet (``read_excel``, as
    ``data.get_dataset_summary``) with the columns ``PAIR_COLUMNS``; ``PID``
    becomes a string (it names a file), the other cells are stripped strings."""
    import pandas as pd
    path = str(path)
    frame = pd.read_csv(path, dtype=str) if path.endswith(".csv") else pd.read_excel(path, dtype=str)
    frame.columns = [str(c).strip() for c in frame.columns]
    missing = [c for c in PAIR_COLUMNS if c not in frame.columns]
    if missing:
        raise ValueError(f"{path}: columns {missing} missing; expected {list(PAIR_COLUMNS)}")
    if not len(frame):
        raise ValueError(f"{path}: no rows")
    for c in PAIR_COLUMNS:
        if frame[c].isna().any():
            raise ValueError(f"{path}: column {c!r} has empty cells")
        frame[c] = frame[c].str.strip()
    if frame["PID"].duplicated().any():
        raise ValueError(f"{path}: PID {sorted(frame['PID'][frame['PID'].duplicated()])} more than once")
    return frame


def compose_pair_metrics(raw, region_keys, affected, weights=None):
    """The metrics of ``test.py:992-1088`` from one pair's raw quantities
    ``raw`` ``[1 + R, 6]`` (``ops.PAIR_RAW``; row 0 the whole latent, row ``1 +
    r`` region ``region_keys[r]``), in float64: ``global_metric = (d_pre -
    d_post) / d_post`` on the Mahalanobis distances, ``global_metric_l2`` the
    same on the Euclidean ones, ``global_metric_directional = |displacement|_M
    cos / d_post``; per affected region ``metric_distances`` and
    ``metric_with_angle`` likewise; ``procedure_metric`` the mean over the
    affected regions of ``w * metric_distances`` (``weights``: region key ->
    the region QDA's accuracy, 1 without)."""
    raw = np.asarray(raw, np.float64)
    if raw.shape != (1 + len(region_keys), 6):
        raise ValueError(f"raw: shape {raw.shape}, expected {(1 + len(region_keys), 6)}")
    if not affected:
        raise ValueError("a procedure affects at least one region")
    with np.errstate(divide="ignore", invalid="ignore"):
        distances = (raw[:, 0] - raw[:, 1]) / raw[:, 1]
        with_angle = raw[:, 5] * raw[:, 4] / raw[:, 1]
        l2 = (raw[0, 2] - raw[0, 3]) / raw[0, 3]
    row = {k: 1 + r for r, k in enumerate(region_keys)}
    procedure = 0.0
    for k in affected:
        procedure += (1 if weights is None else float(weights[str(k)])) * distances[row[k]]
    return {"global_metric": float(distances[0]), "global_metric_l2": float(l2),
            "global_metric_directional": float(with_angle[0]), "procedure_metric": float(procedure / len(affected)),
            "region_metrics": {k: {"metric_distances": float(distances[row[k]]),
                                   "metric_with_angle": float(with_angle[row[k]])} for k in affected}}


class Tester:
    """The reference's ``Tester`` (``test.py:35-56``): ``manager`` a resumed
    :class:`manager.ModelManager`, ``norm_dict`` the ``norm.pt`` dictionary
    (``None`` for un-normalised data), ``train_set`` / ``test_set`` resident
    sets (``data.load_mesh_dataset``), ``out_dir`` the run's folder.  The model
    is put in eval mode; the latent statistics are ``latent_stats``, else
    ``<out_dir>/z_stats.pt``, else computed as ``train.py`` does and written
    there (``compute_latent_stats``, ``test.py:95-117``).  ``seed`` seeds the
    generators :meth:`__call__` hands to its steps, one per step, so a step
    run on its own draws what it draws in the whole run; ``animations`` and
    ``diversity_samples`` are what :meth:`__call__` passes on."""

    def __init__(self, manager, norm_dict, train_set, test_set, out_dir, config, latent_stats=None, seed=0,
                 animations=True, diversity_samples=10000):
        self._manager = manager
        manager.net.eval()
        self._device = manager.device
        self._config = config
        self._normalized_data = bool(config["data"].get("normalize_data", True)) and norm_dict is not None
        self._norm_dict = norm_dict
        self._mean = self._std = None
        if self._normalized_data:
            self._mean = norm_dict["mean"].to(self._device, torch.float32).contiguous()
            self._std = norm_dict["std"].to(self._device, torch.float32).contiguous()
        self._out_dir = str(out_dir)
        os.makedirs(self._out_dir, exist_ok=True)
        self._train_set, self._test_set = train_set, test_set
        self._is_vae = manager.is_vae
        self._swap_features = bool(config["data"].get("swap_features", True))
        self._latent_size = int(config["model"]["latent_size"])
        self.seed, self.animations, self.diversity_samples = int(seed), bool(animations), int(diversity_samples)
        self.latent_stats = self.compute_latent_stats(train_set) if latent_stats is None else \
            {k: v.detach().cpu().float() for k, v in latent_stats.items()}

    # ------------------------------------------------------------ plumbing
    def _path(self, name):
        return os.path.join(self._out_dir, name)

    def _unnormalize_verts(self, verts):
        """``test.py:81-84``."""
        return verts * self._std + self._mean if self._normalized_data else verts

    def _decode(self, z):
        """Decoder output ``[N, V, 3]`` (normalised units) of latents ``[N,
        latent]`` from any device, every chunk of ``manager.generate`` full."""
        z = z.detach().to(self._device, torch.float32)
        n, chunk = z.shape[0], self._manager.bs * self._manager.bs
        pad = -n % chunk
        if pad:
            z = torch.cat([z, z.new_zeros(pad, z.shape[1])])
        return self._manager.generate(z.contiguous())[:n]

    def set_renderings_size(self, size):
        """``test.py:86-87``."""
        self._manager.renderings_size = int(size)

    def set_rendering_background_color(self, color=None):
        """``test.py:89-93``: an ``(r, g, b)`` triple, white by default."""
        self._manager.renderings_background = tuple(float(c) for c in ([1, 1, 1] if color is None else color))

    def compute_latent_stats(self, train_set):
        """``test.py:95-117`` with ``z_stats.pt`` (a dictionary of tensors,
        what ``train.py`` writes) in the place of the reference's pickle."""
        path = self._path("z_stats.pt")
        if os.path.exists(path):
            return torch.load(path, map_location="cpu", weights_only=True)
        stats = self._manager.engine.latent_stats(self._manager.encode(train_set.meshes))
        stats = {k: v.cpu() for k, v in stats.items()}
        torch.save(stats, path)
        return stats

    @property
    def has_classifiers(self):
        m = self._manager
        return getattr(m, "_classifier_params", None) is not None and m.lda._fit is not None \
            and m.qda._fit is not None

    def _need_classifiers(self):
        if not self.has_classifiers:
            raise RuntimeError("no classifiers loaded (a classifier: section and resumed classifier files)")

    # ------------------------------------------------------------ random generation
    def random_latent(self, n, z_range_multiplier=1, generator=None):
        """``test.py:231-242``: a VAE draws ``randn``, an AE uniformly between
        ``mins * m`` and ``maxs * m`` of the latent statistics (CPU tensors)."""
        if self._is_vae:
            return torch.randn([int(n), self._latent_size], generator=generator)
        lo = self.latent_stats["mins"] * z_range_multiplier
        hi = self.latent_stats["maxs"] * z_range_multiplier
        return torch.rand([int(n), lo.shape[0]], generator=generator) * (hi - lo) + lo

    def random_generation(self, n_samples=16, z_range_multiplier=1, denormalize=True, generator=None):
        """``test.py:244-250``: decoded random latents, ``[n, V, 3]`` on the device."""
        gen = self._decode(self.random_latent(n_samples, z_range_multiplier, generator))
        return self._unnormalize_verts(gen) if denormalize else gen

    def random_generation_and_rendering(self, n_samples=16, z_range_multiplier=1, generator=None):
        """``test.py:252-257``: writes ``random_generation.png``."""
        images = self._manager.render(self.random_generation(n_samples, z_range_multiplier, generator=generator))
        grid = rendering.make_grid(images, padding=10, pad_value=1.0)
        return rendering.save_png(self._path("random_generation.png"), grid)

    def random_generation_and_save(self, n_samples=16, z_range_multiplier=1, generator=None):
        """``test.py:259-278``: writes ``random_meshes/<i>.ply`` with the template's faces."""
        out = self._path("random_meshes")
        os.makedirs(out, exist_ok=True)
        verts = self.random_generation(n_samples, z_range_multiplier, generator=generator).cpu().numpy()
        paths = []
        for i in range(verts.shape[0]):
            paths.append(os.path.join(out, f"{i}.ply"))
            precompute.write_ply(paths[-1], verts[i], self._manager.template.faces)
        return paths

    # ------------------------------------------------------------ metrics
    def reconstruction_errors(self, data_set):
        """``test.py:280-301``: eval-mode reconstructions of the set's meshes,
        un-normalised per-vertex errors in mm, their per-mesh means (on the
        device, ``ops.vertex_errors``) and the four summary figures."""
        m = self._manager
        means, rows = [], m.bs * m.bs * 16
        for s in range(0, data_set.meshes.shape[0], rows):
            x = data_set.meshes[s:s + rows].contiguous()
            recon = self._decode(m.encode(x)).contiguous()
            means.append(ops.vertex_errors(recon, x, to_mm=m.to_mm_const, mean=self._mean, std=self._std,
                                           want_mesh_mean=True)[1])
        return ops.reconstruction_error_stats(torch.cat(means))

    def compute_diversity_train_set(self, generator=None):
        """``test.py:303-323``: the training set's base meshes in batches of
        ``batch_size`` -- in stored order, or with ``generator`` in one drawn
        permutation --, the ragged tail dropped; batch ``k`` against batch
        ``k - 1`` mesh by mesh; the mean over all per-mesh mean distances (mm).
        The reference's loader shuffles every time it is walked, so its figure
        and this one are comparable only statistically."""
        m, x = self._manager, self._train_set.meshes
        if generator is not None:
            x = x[torch.randperm(x.shape[0], generator=generator).to(x.device)]
        bs = m.bs
        n = (x.shape[0] // bs) * bs
        if n < 2 * bs:
            raise ValueError(f"{x.shape[0]} training meshes hold fewer than two batches of {bs}")
        means, rows = [], 1024
        for s in range(0, n - bs, rows):
            e = min(s + rows, n - bs)
            means.append(ops.vertex_errors(x[s:e].contiguous(), x[s + bs:e + bs].contiguous(), to_mm=m.to_mm_const,
                                           mean=self._mean, std=self._std, want_mesh_mean=True)[1])
        return torch.mean(torch.cat(means)).item()

    def pair_distances(self, z_a, z_b):
        """Per pair ``(z_a[i], z_b[i])`` the mean distance (mm) between the two
        decoded, un-normalised heads: ``[N]`` on the device.  A pair's figure
        does not depend on the other pairs of the call."""
        if z_a.shape != z_b.shape or z_a.dim() != 2:
            raise ValueError(f"z_a {tuple(z_a.shape)} and z_b {tuple(z_b.shape)}: expected two [N, latent]")
        m, means = self._manager, []
        rows = m.bs * m.bs * 20  # a multiple of the decoder chunk; two such batches of heads are resident
        for s in range(0, z_a.shape[0], rows):
            a, b = self._decode(z_a[s:s + rows]).contiguous(), self._decode(z_b[s:s + rows]).contiguous()
            means.append(ops.vertex_errors(a, b, to_mm=m.to_mm_const, mean=self._mean, std=self._std,
                                           want_mesh_mean=True)[1])
        return torch.cat(means)

    def diversity_of(self, z_a, z_b):
        """The core of :meth:`compute_diversity` with the latents handed in:
        the mean of :meth:`pair_distances` over the pairs, accumulated in
        float64 (exact for fp32 terms), so it does not depend on how the pairs
        are spread over calls or decoder chunks."""
        return float(self.pair_distances(z_a, z_b).double().mean().item())

    def compute_diversity(self, n_samples=10000, generator=None):
        """``test.py:325-334``: ``n_samples // 20`` iterations, each drawing 20
        latents for the first operand, then 20 for the second; the mean
        per-mesh distance (mm) over all ``(n_samples // 20) * 20`` pairs."""
        iters = int(n_samples) // 20
        if iters < 1:
            raise ValueError(f"n_samples {n_samples} < 20")
        z_a, z_b = [], []
        for _ in range(iters):
            z_a.append(self.random_latent(20, generator=generator))
            z_b.append(self.random_latent(20, generator=generator))
        return self.diversity_of(torch.cat(z_a), torch.cat(z_b))

    # ------------------------------------------------------------ traversals
    def traversal_latents(self, z_range_multiplier=1, use_z_stats=True, n_steps=N_STEPS):
        """``test.py:130-150``: ``[latent, n_steps, latent]`` (CPU); row ``i``
        is the mean latent repeated with column ``i`` running over
        ``torch.linspace(z_mins[i], z_maxs[i], n_steps)``.  A VAE with
        ``use_z_stats=False``: means 0, range ``+-3 * multiplier``; otherwise
        the latent statistics, mins and maxs times the multiplier."""
        if self._is_vae and not use_z_stats:
            means = torch.zeros(self._latent_size)
            mins = -3 * z_range_multiplier * torch.ones(self._latent_size)
            maxs = 3 * z_range_multiplier * torch.ones(self._latent_size)
        else:
            means = self.latent_stats["means"]
            mins = self.latent_stats["mins"] * z_range_multiplier
            maxs = self.latent_stats["maxs"] * z_range_multiplier
        out = means.repeat(means.shape[0], int(n_steps), 1)
        for i in range(means.shape[0]):
            out[i, :, i] = torch.linspace(mins[i], maxs[i], int(n_steps))
        return out

    def latent_traversals(self, z_range_multiplier=1, use_z_stats=True, save_suffix=None, animations=True,
                          latents=None, n_steps=N_STEPS):
        """``test.py:128-229``: every latent variable (or the indices
        ``latents``) walked from its minimum to its maximum in ``n_steps``
        frames.  All frames are decoded and un-normalised, their distance to
        their traversal's first frame comes from ``ops.group_vertex_errors``,
        ``max_distances`` ``[G, V]`` is each traversal's last frame and
        ``ops.region_means`` of it the ``[G, R]`` table of the reference's two
        seaborn plots.  Writes ``latent_exploration_tiled{s}.png`` (the last
        step's error maps), ``latent_exploration{s}.json`` (the table) and,
        with ``animations``, three animated PNGs with the frames of the
        reference's three videos: ``latent_exploration{s}.apng`` (rendering |
        error map per step, two black frames after each latent, 4 fps),
        ``latent_exploration_tiled{s}.apng`` (the error maps of every latent
        in one grid per step, 1 fps) and ``latent_exploration_out_tiled{s}.apng``
        (the renderings likewise, 4 fps).  Without ``animations`` only the last
        step is drawn.  Returns ``{"table", "max_distances", "latents",
        "regions", "files"}``."""
        m, n = self._manager, int(n_steps)
        all_z = self.traversal_latents(z_range_multiplier, use_z_stats, n)
        which = list(range(all_z.shape[0])) if latents is None else [int(i) for i in latents]
        groups = len(which)
        gen = self._unnormalize_verts(self._decode(all_z[which].reshape(groups * n, -1))).contiguous()
        diffs = ops.group_vertex_errors(gen, n, to_mm=m.to_mm_const)
        max_distances = diffs.view(groups, n, -1)[:, -1].contiguous()
        table = ops.region_means(max_distances, m.topology.region_csr)
        s = save_suffix if save_suffix is not None else ""
        nrow = self._latent_size // len(m.latent_regions) if self._swap_features else 8
        files = {}

        def grid(images):
            return rendering.make_grid(images, nrow=nrow, padding=10, pad_value=255)

        if animations:
            shots, maps = self._traversal_pictures(gen, diffs, groups, n)
            frames = torch.cat([shots, maps], dim=-1)
            frames = torch.cat([frames, torch.zeros_like(frames[:, :2])], dim=1).flatten(0, 1)
            files["animation"] = rendering.save_apng(self._path(f"latent_exploration{s}.apng"), frames, fps=4)
            tiled = torch.stack([grid(maps[:, i]) for i in range(n)])
            files["tiled_animation"] = rendering.save_apng(self._path(f"latent_exploration_tiled{s}.apng"), tiled,
                                                           fps=1)
            out_tiled = torch.stack([grid(shots[:, i]) for i in range(n)])
            files["out_tiled_animation"] = rendering.save_apng(self._path(f"latent_exploration_out_tiled{s}.apng"),
                                                               out_tiled, fps=4)
            last = tiled[-1]
        else:
            last_frames = gen.view(groups, n, -1, 3)[:, -1].contiguous()
            last = grid(torch.cat([_quantise(m.render(last_frames[g:g + 25], max_distances[g:g + 25], error_max_scale=5))
                                   for g in range(0, groups, 25)]))
        files["tiled"] = rendering.save_png(self._path(f"latent_exploration_tiled{s}.png"), last)
        regions = [str(k) for k in (m.topology.region_keys or range(table.shape[1]))]
        files["table"] = _dump(self._path(f"latent_exploration{s}.json"),
                               {"regions": regions, "latents": which, "mean_dist": table.cpu().tolist()})
        return {"table": table, "max_distances": max_distances, "latents": which, "regions": regions, "files": files}

    def _traversal_pictures(self, gen, diffs, groups, n):
        """Renderings and error maps (over [0, 5] mm) of every traversal frame,
        quantised: two uint8 device tensors ``[G, n, 3, S, S]``.  One traversal
        per launch set: the raster workspace stays small."""
        m, shots, maps = self._manager, [], []
        for g in range(groups):
            sl = slice(g * n, (g + 1) * n)
            shots.append(_quantise(m.render(gen[sl])))
            maps.append(_quantise(m.render(gen[sl], diffs[sl], error_max_scale=5)))
        return torch.stack(shots), torch.stack(maps)

    # ------------------------------------------------------------ interpolation
    vector_linspace = staticmethod(vector_linspace)

    def _default_interpolation_pair(self):
        """The first non-augmented test mesh and the non-augmented test mesh
        with the largest MSE to it (``test.py:552-569``), un-normalised; read
        from the resident test set, not from the files again."""
        ts = self._test_set
        labels = getattr(ts, "labels", None)
        keep = [i for i in range(ts.meshes.shape[0]) if labels is None or not labels[i][1]]
        if len(keep) < 2:
            raise ValueError("the test set holds fewer than two non-augmented meshes")
        x = self._unnormalize_verts(ts.meshes[torch.tensor(keep, device=ts.meshes.device)])
        mse = ((x - x[0]) ** 2).mean(dim=(1, 2))
        return x[0], x[int(mse.argmax().item())]

    def interpolate(self, v_1=None, v_2=None, animations=True):
        """``test.py:544-637`` between two un-normalised meshes ``[V, 3]``
        (default: :meth:`_default_interpolation_pair`), three schedules.  Per
        feature (only with ``swap_features``): region after region, that
        region's latent slice moves from mesh 1 to mesh 2 in ``len(features)
        // 2`` steps, the last row carried into the next region; one grid row
        per region -> ``interpolate_per_feature.png`` (+ ``.apng``, 4 fps).
        Per variable: one latent variable at a time in 3 steps, carrying the
        last row -> ``interpolate_per_variable.apng``.  All features at once in
        ``len(features)`` steps -> ``interpolate_all.png``."""
        m = self._manager
        if v_1 is None or v_2 is None:
            d_1, d_2 = self._default_interpolation_pair()
            v_1, v_2 = (d_1 if v_1 is None else v_1), (d_2 if v_2 is None else v_2)
        zs = []
        for v in (v_1, v_2):
            v = torch.as_tensor(v, dtype=torch.float32).to(self._device)
            if self._normalized_data:
                v = (v - self._mean) / self._std
            zs.append(m.encode(v.unsqueeze(0).contiguous()).cpu())
        z_1, z_2 = zs
        features = list(m.latent_regions)
        n_f = len(features)
        files = {}

        def shots(z):
            return m.render(self._unnormalize_verts(self._decode(z)))

        if self._swap_features:
            steps = n_f // 2
            z = z_1.repeat(steps, 1)
            frames, rows = [], []
            for feature in features:
                lo, hi = m.latent_regions[feature]
                z[:, lo:hi] = vector_linspace(z_1[:, lo:hi], z_2[:, lo:hi], steps)
                r = shots(z)
                frames.append(r)
                rows.append(rendering.make_grid(r, padding=10, pad_value=1.0, nrow=n_f))
                z = z[-1, :].repeat(steps, 1)
            files["per_feature"] = rendering.save_png(self._path("interpolate_per_feature.png"),
                                                      torch.cat(rows, dim=-2))
            if animations:
                files["per_feature_animation"] = rendering.save_apng(self._path("interpolate_per_feature.apng"),
                                                                     torch.cat(frames), fps=4)
        if animations:
            z = z_1.repeat(3, 1)
            all_z = []
            for i in range(self._latent_size):
                z[:, i] = torch.linspace(z_1[0, i].item(), z_2[0, i].item(), 3)
                all_z.append(z)
                z = z[-1, :].repeat(3, 1)
            files["per_variable_animation"] = rendering.save_apng(self._path("interpolate_per_variable.apng"),
                                                                  shots(torch.cat(all_z)), fps=4)
        grid = rendering.make_grid(shots(vector_linspace(z_1, z_2, n_f)), padding=10, pad_value=1.0, nrow=n_f)
        files["all"] = rendering.save_png(self._path("interpolate_all.png"), grid)
        return files

    # ------------------------------------------------------------ classifiers
    def _latents_and_labels(self, data_set):
        m = self._manager
        z = m.encode(data_set.meshes).contiguous()
        letters = [lab[0] for lab in data_set.labels]
        aug = np.array([bool(lab[1]) for lab in data_set.labels])
        return z, letters, aug

    def embeddings(self, mode="lda"):
        """The numbers behind ``plot_embeddings`` (``test.py:1161-1321``):
        the 2-D LDA projection of the train and test latents and, per latent
        region, the region LDA's projection of the training latents (a region
        of one or two variables: its first and last variable).  Writes
        ``lda_embeddings.npz``: ``x1``, ``x2``, ``class``, ``is_test``,
        ``augmented`` over train then test rows, ``region_keys`` and one
        ``region_<i>`` ``[N_train, 2]`` per region."""
        if mode == "tsne":
            raise NotImplementedError("embeddings() draws the LDA projection and needs classifiers; "
                                      "the t-SNE embedding is tsne_embeddings()")
        if mode != "lda":
            raise NotImplementedError(f"embedding mode {mode!r}")
        self._need_classifiers()
        m = self._manager
        tr_z, tr_l, tr_a = self._latents_and_labels(self._train_set)
        ts_z, ts_l, ts_a = self._latents_and_labels(self._test_set)
        xy = torch.cat([m.lda_project_latents_in_2d(tr_z), m.lda_project_latents_in_2d(ts_z)]).cpu().numpy()
        out = {"x1": xy[:, 0], "x2": xy[:, -1], "class": np.array(tr_l + ts_l),
               "is_test": np.array([False] * len(tr_l) + [True] * len(ts_l)), "augmented": np.concatenate([tr_a, ts_a]),
               "region_keys": np.array([str(k) for k in m.latent_regions])}
        for i, (key, (lo, hi)) in enumerate(m.latent_regions.items()):
            if hi - lo > 2 and m.region_ldas is not None:
                e = m.region_ldas[key].transform(tr_z)
                e = torch.stack([e[:, 0], e[:, -1]], dim=1)
            else:
                e = torch.stack([tr_z[:, lo], tr_z[:, hi - 1]], dim=1)
            out[f"region_{i}"] = e.cpu().numpy()
        path = self._path("lda_embeddings.npz")
        np.savez(path, **out)
        return path

    def tsne_embeddings(self, perplexity=30.0, generator=None):
        """The points of ``plot_embeddings``'s other branch (``test.py:1177-1180``:
        ``TSNE(n_components=2, init='random')`` of the train and test
        latents), embedded on the device by :func:`tsne.fit_transform`; no
        classifiers are needed.  Writes ``tsne_embeddings.npz``: ``x1``,
        ``x2``, ``class``, ``is_test``, ``augmented`` over train then test rows
        (the rows of ``lda_embeddings.npz``), ``kl_divergence``, ``n_iter`` and
        ``perplexity``.  ``generator``: the CPU ``torch.Generator`` of the
        random initial embedding."""
        tr_z, tr_l, tr_a = self._latents_and_labels(self._train_set)
        ts_z, ts_l, ts_a = self._latents_and_labels(self._test_set)
        fit = tsne.fit_transform(torch.cat([tr_z, ts_z]).contiguous(), perplexity=perplexity, generator=generator)
        xy = fit.y.cpu().numpy()
        path = self._path("tsne_embeddings.npz")
        np.savez(path, x1=xy[:, 0], x2=xy[:, 1], **{"class": np.array(tr_l + ts_l)},
                 is_test=np.array([False] * len(tr_l) + [True] * len(ts_l)), augmented=np.concatenate([tr_a, ts_a]),
                 kl_divergence=np.float64(fit.kl_divergence), n_iter=np.int64(fit.n_iter),
                 perplexity=np.float64(perplexity))
        return path

    def test_classifiers(self):
        """``test.py:1323-1419`` without the SVM and the plots: the test
        accuracies of the MLP (per cent, the mean over the batches of
        ``mlp_classifier_epoch``), LDA and QDA (fractions, ``score``) ->
        ``accuracies.json``; their classification reports ->
        ``classification_report.json``; the row-normalised confusion matrices
        with their labels -> ``confusion_matrices.json``; per region the QDA's
        report with its ``score`` as ``accuracy`` ->
        ``classification_report_regions.json`` and the LDA's / QDA's confusion
        matrices -> ``region_confusion_matrices.json`` (the last two only with
        region classifiers).  Returns the accuracies."""
        self._need_classifiers()
        from .classify import count_labels
        m = self._manager
        if m._class_weights is None:
            m.set_class_conversions_and_weights(count_labels(self._train_set.labels))
        z, letters, _ = self._latents_and_labels(self._test_set)
        y = torch.tensor(m.class2idx(letters), dtype=torch.int32).to(self._device)
        acc = {"accuracy_mlp": float(m.classifier_mlp.run_epoch(z, y, m._class_weights, m.bs, train=False)[1]),
               "accuracy_lda": m.lda.score(z, y), "accuracy_qda": m.qda.score(z, y)}
        files = {"accuracies": _dump(self._path("accuracies.json"), acc)}
        pred = {"mlp": m.idx2class(m.classifier_mlp(z)[1]), "lda": m.idx2class(m.lda.predict(z)),
                "qda": m.idx2class(m.qda.predict(z))}
        files["report"] = _dump(self._path("classification_report.json"),
                                {k: classification_report(letters, p) for k, p in pred.items()})
        cms = {k: {"labels": _labels_of(letters, p), "matrix": confusion_matrix(letters, p, "true").tolist()}
               for k, p in pred.items()}
        files["confusion"] = _dump(self._path("confusion_matrices.json"), cms)
        if m.region_qdas is not None:
            reports, region_cms = {}, {"lda": {}, "qda": {}}
            for key in m.latent_regions:
                p_qda = m.idx2class(m.region_qdas[key].predict(z))
                reports[str(key)] = classification_report(letters, p_qda)
                reports[str(key)]["accuracy"] = m.region_qdas[key].score(z, y)
                for kind, p in (("lda", m.idx2class(m.region_ldas[key].predict(z))), ("qda", p_qda)):
                    region_cms[kind][str(key)] = {"labels": _labels_of(letters, p),
                                                  "matrix": confusion_matrix(letters, p, "true").tolist()}
            files["region_reports"] = _dump(self._path("classification_report_regions.json"), reports)
            files["region_confusion"] = _dump(self._path("region_confusion_matrices.json"), region_cms)
        self.classifier_files = files
        return acc

    # ------------------------------------------------------------ surgical planning
    def _load_and_encode(self, mesh_path):
        """``test.py:637-650``: the latent ``[1, latent]`` (device) of the mesh
        file ``mesh_path``, normalised as the training data was."""
        from .data import load_mesh
        v = load_mesh(str(mesh_path)).to(self._device, torch.float32)
        if self._normalized_data:
            v = (v - self._mean) / self._std
        return self._manager.encode(v.unsqueeze(0).contiguous()).contiguous()

    @staticmethod
    def _mesh_id(mesh_path):
        return os.path.splitext(os.path.basename(str(mesh_path)))[0]

    def _region_projections(self, z):
        """Per latent region the region LDA's first and last component of the
        latents ``z`` ``[N, latent]``: ``{str(key): [[x1, x2], ...]}`` (empty
        without region classifiers)."""
        m = self._manager
        if m.region_ldas is None:
            return {}
        out = {}
        for key in m.latent_regions:
            e = m.region_ldas[key].transform(z)
            out[str(key)] = torch.stack([e[:, 0], e[:, -1]], dim=1).cpu().tolist()
        return out

    def plan_to_normal(self, z, levels=PLAN_LEVELS, steps=PLAN_STEPS, n_first=PLAN_FIRST):
        """The planning arithmetic of ``test.py:663-740`` for the latents ``z``
        ``[n, latent]`` (device): the crossings of each path to the mean of
        the main QDA's class ``n`` (``ops.plan_targets``) and the latent tables
        of moving every region and of each procedure of
        :func:`planning_procedures` (``ops.plan_tables``).  Returns ``{"maha"
        [n], "index" [n, S], "targets" [n, S + 1, latent], "tables" [n, 1 + P,
        n_first + S, latent], "dist" [n, 1 + P, S + 1], "groups"}``, ``groups``
        naming the 1 + P groups (``all_attributes`` first)."""
        self._need_classifiers()
        m = self._manager
        mean, whiten, _ = m.qda_gaussian("n")
        z = z.detach().to(self._device, torch.float32).contiguous()
        maha, index, targets = ops.plan_targets(z, mean, whiten, levels, steps)
        procedures = planning_procedures(self._config, m.latent_regions)
        mask = torch.zeros((len(procedures), z.shape[1]), dtype=torch.uint8)
        for p, keys in enumerate(procedures.values()):
            for key in keys:
                lo, hi = m.latent_regions[key]
                mask[p, lo:hi] = 1
        tables, dist = ops.plan_tables(z, targets, mask.to(self._device) if len(procedures) else None, n_first)
        return {"maha": maha, "index": index, "targets": targets, "tables": tables, "dist": dist,
                "groups": ["all_attributes"] + list(procedures)}

    def interpolate_syndrome_to_normal(self, patient_path, animations=True):
        """``test.py:652-870``: the patient's latent moved to the healthy
        distribution, in every region and in the regions of each procedure
        (:meth:`plan_to_normal`); all ``(1 + P) * F`` latents decoded at once,
        their distance to their group's first frame from
        ``ops.group_vertex_errors``, rendered at 512 pixels on white, plain
        and as an error map over [0, 10] mm.  Per group, under
        ``interpolations/<id>_<name>/``: ``meshes/<i>.ply`` and
        ``meshes_colormap/<i>.ply`` (plasma vertex colours),
        ``<id>_<name>_interpolate.png`` (renderings above error maps, one
        column per frame, padding 10), ``.apng`` (rendering | error map, 4
        fps; with ``animations``) and ``embedding.json`` (``lda``: the 2-D LDA
        projection of the ``F`` latents, ``regions``: each region LDA's, the
        points the reference scatters into its pickled figures).
        ``interpolations/<id>_procedure_distances.csv`` lists ``procedure, d3,
        d2, d1, dm`` per procedure.  Returns the dictionary of
        :meth:`plan_to_normal` plus ``frames`` ``[(1 + P) * F, V, 3]``,
        ``errors`` ``[(1 + P) * F, V]`` and ``files``."""
        m = self._manager
        pid = self._mesh_id(patient_path)
        plan = self.plan_to_normal(self._load_and_encode(patient_path))
        groups = plan["groups"]
        n_groups, n_frames, latent = plan["tables"].shape[1:]
        z_all = plan["tables"].view(n_groups * n_frames, latent)
        frames = self._unnormalize_verts(self._decode(z_all)).contiguous()
        errors = ops.group_vertex_errors(frames, n_frames, to_mm=m.to_mm_const)
        colours = (rendering.errors_to_colors(errors, 0, 10) * 255.0 + 0.5).to(torch.uint8)
        colours = torch.cat([colours, torch.full_like(colours[..., :1], 255)], dim=-1).cpu().numpy()
        verts = frames.cpu().numpy()
        lda_xy = m.lda_project_latents_in_2d(z_all)
        lda_xy = torch.stack([lda_xy[:, 0], lda_xy[:, -1]], dim=1).cpu().tolist()
        region_xy = self._region_projections(z_all)
        root = self._path("interpolations")
        size, background = m.renderings_size, m.renderings_background
        self.set_renderings_size(512)
        self.set_rendering_background_color([1, 1, 1])
        files = {}
        try:
            for g, name in enumerate(groups):
                sl = slice(g * n_frames, (g + 1) * n_frames)
                save_id = f"{pid}_{name}"
                out = os.path.join(root, save_id)
                for sub in ("meshes", "meshes_colormap"):
                    os.makedirs(os.path.join(out, sub), exist_ok=True)
                for i in range(n_frames):
                    precompute.write_ply(os.path.join(out, "meshes", f"{i}.ply"), verts[sl][i], m.template.faces)
                    precompute.write_ply(os.path.join(out, "meshes_colormap", f"{i}.ply"), verts[sl][i],
                                         m.template.faces, colours[sl][i])
                shots = m.render(frames[sl])
                maps = m.render(frames[sl], errors[sl], error_max_scale=10)
                grid = rendering.make_grid(torch.cat([shots, maps], dim=-2), padding=10, pad_value=1.0, nrow=n_frames)
                files[name] = {"picture": rendering.save_png(os.path.join(out, save_id + "_interpolate.png"), grid)}
                if animations:
                    files[name]["animation"] = rendering.save_apng(os.path.join(out, save_id + "_interpolate.apng"),
                                                                   torch.cat([shots, maps], dim=-1), fps=4)
                files[name]["embedding"] = _dump(os.path.join(out, "embedding.json"), {
                    "lda": lda_xy[sl], "regions": {k: v[sl] for k, v in region_xy.items()}})
        finally:
            m.renderings_size, m.renderings_background = size, background
        dist = plan["dist"][0].cpu().numpy().astype(np.float64)
        files["distances"] = os.path.join(root, f"{pid}_procedure_distances.csv")
        with open(files["distances"], "w") as f:
            f.write("procedure,d3,d2,d1,dm\n")
            for g, name in enumerate(groups[1:], start=1):
                f.write(name + "," + ",".join(repr(float(v)) for v in dist[g]) + "\n")
        return {**plan, "frames": frames, "errors": errors, "files": files}

    def classify_and_project(self, patient_path):
        """``test.py:872-904``: the QDA's class of the patient, its 2-D LDA
        point and each region LDA's point, returned and written to
        ``interpolations/<id>_emb.json`` (``class``, ``lda``, ``regions``)."""
        self._need_classifiers()
        m = self._manager
        z = self._load_and_encode(patient_path)
        xy = m.lda_project_latents_in_2d(z)
        out = {"class": m.classify_latent(z, "qda")[0], "lda": [float(xy[0, 0]), float(xy[0, -1])],
               "regions": {k: v[0] for k, v in self._region_projections(z).items()}}
        os.makedirs(self._path("interpolations"), exist_ok=True)
        _dump(os.path.join(self._path("interpolations"), self._mesh_id(patient_path) + "_emb.json"), out)
        return out

    def _pair_windows(self):
        """The windows of ``ops.pair_metrics``: row 0 the whole latent under
        the main QDA's healthy class, rows ``1..R`` the latent regions under
        their own QDAs (none without region classifiers).  Returns ``(region
        keys, windows, packed mean, packed whiten)``."""
        m = self._manager
        keys = list(m.latent_regions) if m.region_qdas is not None else []
        windows, means, whitens, n_mean, n_whiten = [], [], [], 0, 0
        for key in ["all"] + keys:
            mean, whiten, cols = m.qda_gaussian("n", region=key)
            col0, d = (0, mean.shape[0]) if cols is None else cols
            windows.append((col0, d, n_mean, n_whiten))
            means.append(mean)
            whitens.append(whiten.reshape(-1))
            n_mean, n_whiten = n_mean + d, n_whiten + d * d
        return keys, windows, torch.cat(means).contiguous(), torch.cat(whitens).contiguous()

    def _region_weights(self):
        """``classification_report_regions.json`` of :meth:`test_classifiers`:
        region key -> the region QDA's accuracy, or None (then the procedure
        metric is not weighted, ``test.py:1024-1032``)."""
        try:
            with open(self._path("classification_report_regions.json")) as f:
                return {k: float(v["accuracy"]) for k, v in json.load(f).items()}
        except FileNotFoundError:
            print("procedure specific metric not weighted according to local QDA performance. "
                  "Test classifiers first!", flush=True)
            return None

    def pre_post_metrics(self, z_pre, z_post, patient_ids, procedures):
        """:meth:`evaluate_pre_post_pair` for ``N`` encoded pairs: ONE
        ``ops.pair_metrics`` call over every pair and window, everything after
        it float64 on the host.  ``procedures``: per pair a name of
        :func:`planning_procedures`.  Writes ``pre_post_eval/<pid>.json`` per
        pair and returns the list of dictionaries (``raw`` ``[1 + R, 6]``
        among their entries)."""
        self._need_classifiers()
        m = self._manager
        table = planning_procedures(self._config, m.latent_regions)
        unknown = sorted({str(p) for p in procedures} - set(table))
        if unknown:
            raise ValueError(f"procedure(s) {unknown} not among {sorted(table)} (planning.procedures)")
        keys, windows, mean, whiten = self._pair_windows()
        if not keys:
            raise RuntimeError("the pre- / post-operative metrics need the region classifiers "
                               "(latent_consistency_weight > 0)")
        z_pre = z_pre.detach().to(self._device, torch.float32).contiguous()
        z_post = z_post.detach().to(self._device, torch.float32).contiguous()
        raw = ops.pair_metrics(z_pre, z_post, windows, mean, whiten).cpu().numpy().astype(np.float64)
        weights = self._region_weights()
        classes = [m.classify_latent(z, "qda") for z in (z_pre, z_post)]
        posteriors = [torch.softmax(m.qda.decision_function(z).double(), dim=1).cpu().tolist() for z in (z_pre, z_post)]
        lda = [m.lda_project_latents_in_2d(z) for z in (z_pre, z_post)]
        lda = [torch.stack([e[:, 0], e[:, -1]], dim=1).cpu().tolist() for e in lda]
        os.makedirs(self._path("pre_post_eval"), exist_ok=True)
        results = []
        for i, (pid, procedure) in enumerate(zip(patient_ids, procedures)):
            out = {"pre_class": classes[0][i], "post_class": classes[1][i],
                   **compose_pair_metrics(raw[i], keys, table[str(procedure)], weights)}
            out["region_metrics"] = {str(k): v for k, v in out["region_metrics"].items()}
            out.update(patient_id=str(pid), procedure=str(procedure), pre_posteriors=posteriors[0][i],
                       post_posteriors=posteriors[1][i], pre_lda=lda[0][i], post_lda=lda[1][i], raw=raw[i].tolist())
            _dump(os.path.join(self._path("pre_post_eval"), f"{pid}.json"), out)
            results.append(out)
        return results

    def evaluate_pre_post_pair(self, pre_path, post_path, patient_id, procedure):
        """``test.py:972-1088``: the surgical-effectiveness metrics of one
        pre- / post-operative pair of mesh files for ``procedure`` (a name of
        :func:`planning_procedures`).  Returns the reference's dictionary
        (``pre_class``, ``post_class``, ``global_metric``,
        ``global_metric_l2``, ``global_metric_directional``,
        ``procedure_metric``, ``region_metrics``) with the QDA posteriors
        (``softmax`` of ``decision_function``), the 2-D LDA projections of
        both latents and the raw quantities, and writes it to
        ``pre_post_eval/<patient_id>.json``."""
        return self.pre_post_metrics(self._load_and_encode(pre_path), self._load_and_encode(post_path),
                                     [patient_id], [procedure])[0]

    def evaluate_all_pre_post_pairs(self, pairs_root, pairs_table):
        """``test.py:906-970`` without the plots: every row of ``pairs_table``
        (:func:`read_pairs_table`; ``Surgery regions`` names the procedure)
        encoded from ``pairs_root`` and evaluated in one
        :meth:`pre_post_metrics` call.  Writes
        ``pre_post_eval/<table>_with_results.csv`` (the table plus the scalar
        metrics) and ``pre_post_eval/region_metrics.json`` (per row
        ``Procedure``, ``Syndrome`` and the two per-region metrics: the
        numbers behind the reference's three box plots).  Returns the list of
        per-pair dictionaries."""
        frame = read_pairs_table(pairs_table)
        z_pre = torch.cat([self._load_and_encode(os.path.join(str(pairs_root), n)) for n in frame["Pre name"]])
        z_post = torch.cat([self._load_and_encode(os.path.join(str(pairs_root), n)) for n in frame["Post name"]])
        results = self.pre_post_metrics(z_pre, z_post, list(frame["PID"]), list(frame["Surgery regions"]))
        scalars = ("pre_class", "post_class", "global_metric", "global_metric_l2", "global_metric_directional",
                   "procedure_metric")
        for k in scalars:
            frame[k] = [r[k] for r in results]
        stem = os.path.splitext(os.path.basename(str(pairs_table)))[0]
        frame.to_csv(os.path.join(self._path("pre_post_eval"), stem + "_with_results.csv"), index=False)
        rows = [{"PID": r["patient_id"], "Procedure": proc, "Syndrome": syn,
                 "metric_distances": {k: v["metric_distances"] for k, v in r["region_metrics"].items()},
                 "metric_with_angle": {k: v["metric_with_angle"] for k, v in r["region_metrics"].items()}}
                for r, proc, syn in zip(results, frame["Procedure"], frame["Syndrome"])]
        _dump(os.path.join(self._path("pre_post_eval"), "region_metrics.json"), {"rows": rows})
        return results

    def save_postop_colourmap(self, pre_path, post_path):
        """``compute_and_save_postop_mesh_colourmap`` (``test.py:1138-1151``):
        the post-operative mesh coloured by its per-vertex distance to the
        pre-operative one (``ops.vertex_errors``, plasma over [0, 10] mm),
        written next to it as ``<post>_colmap.ply``."""
        from .data import load_mesh
        m = self._manager
        pre = load_mesh(str(pre_path)).to(self._device).unsqueeze(0).contiguous()
        post = load_mesh(str(post_path)).to(self._device).unsqueeze(0).contiguous()
        dist = ops.vertex_errors(post, pre, to_mm=m.to_mm_const)
        colours = (rendering.errors_to_colors(dist[0], 0, 10) * 255.0 + 0.5).to(torch.uint8)
        colours = torch.cat([colours, torch.full_like(colours[:, :1], 255)], dim=-1).cpu().numpy()
        path = os.path.splitext(str(post_path))[0] + "_colmap.ply"
        precompute.write_ply(path, post[0].cpu().numpy(), m.template.faces, colours)
        return path

    # ------------------------------------------------------------ the embedding figures
    def embedding_figures(self, mode="lda"):
        """``plot_embeddings`` and ``plot_embeddings_per_region``
        (``test.py:1161-1321``) drawn by :func:`figures.embedding_figures`.
        ``lda``: the arrays :meth:`embeddings` writes (needs classifiers), files
        ``lda_emb_*.png``, ``emb_all_train.png`` and ``emb_all_train_dist.png``;
        ``tsne``: the points of ``tsne_embeddings.npz`` (fitted by
        :meth:`tsne_embeddings` when the file is not there), prefix ``tsne``, no
        region figure, no classifiers.  Returns the base images and layouts,
        which are kept in ``figure_bases[mode]`` for :meth:`plan_figures` and
        :meth:`prepost_figures`."""
        if mode == "lda":
            data = np.load(self.embeddings())
            regions = {str(k): data[f"region_{i}"] for i, k in enumerate(data["region_keys"])}
        elif mode == "tsne":
            path = self._path("tsne_embeddings.npz")
            data = np.load(path if os.path.exists(path) else self.tsne_embeddings(generator=self._generator(5)))
            regions = None
        else:
            raise NotImplementedError(f"embedding mode {mode!r}")
        xy = np.stack([data["x1"], data["x2"]], axis=1)
        out = figures.embedding_figures(xy, data["class"], data["is_test"], data["augmented"], self._out_dir,
                                        prefix=mode, regions=regions, device=self._device)
        self.figure_bases = {**self.figure_bases, mode: out}
        return out

    def _lda_bases(self):
        bases = self.figure_bases.get("lda") or self.embedding_figures("lda")
        return bases["distributions"], bases.get("all_train_dist")

    def _lda_points(self, z):
        xy = self._manager.lda_project_latents_in_2d(z)
        return torch.stack([xy[:, 0], xy[:, -1]], dim=1).cpu().tolist()

    def plan_figures(self, patient_path, animations=None):
        """``_render_embed_save_z_interpolations`` (``test.py:750-833``): the
        path of :meth:`plan_to_normal` scattered on the density maps.  Per group,
        under ``interpolations/<id>_<name>/``: ``<id>_<name>_emb_interpolate.png``
        (every point of the path on ``lda_emb_distributions.png``),
        ``<id>_<name>_emb_r_interpolate.png`` (each region LDA's points on
        ``emb_all_train_dist.png``; with region classifiers) and, with
        animations, the two ``.apng`` at 4 fps, one point per frame.  Returns
        ``{group: {file kind: path}}``."""
        self._need_classifiers()
        animations = self.animations if animations is None else animations
        main, regional = self._lda_bases()
        pid = self._mesh_id(patient_path)
        plan = self.plan_to_normal(self._load_and_encode(patient_path))
        n_groups, n_frames, latent = plan["tables"].shape[1:]
        z_all = plan["tables"].view(n_groups * n_frames, latent)
        lda_xy, region_xy = self._lda_points(z_all), self._region_projections(z_all)
        files = {}
        for g, name in enumerate(plan["groups"]):
            rows = range(g * n_frames, (g + 1) * n_frames)
            save_id = f"{pid}_{name}"
            out = os.path.join(self._path("interpolations"), save_id)
            os.makedirs(out, exist_ok=True)
            sheets = [("emb", main, [[{"panel": 0, "kind": "disc", "xy": lda_xy[r], "colour": figures.PATH_COLOUR}]
                                     for r in rows])]
            if regional is not None and region_xy:
                sheets.append(("emb_r", regional, [[{"panel": k, "kind": "disc", "xy": v[r],
                                                     "colour": figures.PATH_COLOUR} for k, v in region_xy.items()]
                                                   for r in rows]))
            files[name] = {}
            for tag, base, frames in sheets:
                whole = figures.overlay(base["image"], base["layout"], [[m for f in frames for m in f]])
                files[name][tag] = rendering.save_png(os.path.join(out, f"{save_id}_{tag}_interpolate.png"), whole[0])
                if animations:
                    files[name][tag + "_animation"] = rendering.save_apng(
                        os.path.join(out, f"{save_id}_{tag}_interpolate.apng"),
                        figures.overlay(base["image"], base["layout"], frames), fps=4)
        return files

    def prepost_figures(self, z_pre, z_post, patient_ids):
        """``_project_pre_post_pair`` (``test.py:1090-1136``): per patient
        ``pre_post_eval_plots/<pid>_emb.png`` (on ``lda_emb_distributions.png``)
        and, with region classifiers, ``<pid>_emb_r.png`` (on
        ``emb_all_train_dist.png``): the pre-operative point, the
        post-operative point and an arrow from the first to the second.
        Returns ``{pid: {file kind: path}}``."""
        self._need_classifiers()
        main, regional = self._lda_bases()
        z_pre = z_pre.detach().to(self._device, torch.float32).contiguous()
        z_post = z_post.detach().to(self._device, torch.float32).contiguous()
        if z_pre.shape != z_post.shape or len(patient_ids) != len(z_pre):
            raise ValueError(f"z_pre {tuple(z_pre.shape)}, z_post {tuple(z_post.shape)} and {len(patient_ids)} ids "
                             "must name the same pairs")
        out = self._path("pre_post_eval_plots")
        os.makedirs(out, exist_ok=True)

        def pair(panel, a, b):
            return [{"panel": panel, "kind": "arrow", "xy": a, "xy2": b, "colour": figures.POST_COLOUR},
                    {"panel": panel, "kind": "disc", "xy": a, "colour": figures.PRE_COLOUR},
                    {"panel": panel, "kind": "disc", "xy": b, "colour": figures.POST_COLOUR}]

        sheets = [("emb", main, [pair(0, a, b) for a, b in zip(self._lda_points(z_pre), self._lda_points(z_post))])]
        r_pre, r_post = self._region_projections(z_pre), self._region_projections(z_post)
        if regional is not None and r_pre:
            sheets.append(("emb_r", regional, [[m for k in r_pre for m in pair(k, r_pre[k][i], r_post[k][i])]
                                               for i in range(len(patient_ids))]))
        files = {str(pid): {} for pid in patient_ids}
        for tag, base, frames in sheets:
            images = figures.overlay(base["image"], base["layout"], frames)
            for i, pid in enumerate(patient_ids):
                files[str(pid)][tag] = rendering.save_png(os.path.join(out, f"{pid}_{tag}.png"), images[i])
        return files

    def all_figures(self):
        """The step ``figures``: the LDA embedding figures with classifiers
        (the t-SNE ones without), the plan figures of every mesh of
        ``plan_patients`` and, with ``pairs_table`` and ``pairs_root``, the pair
        figures of every row of the table."""
        if not self.has_classifiers:
            return {"tsne": self.embedding_figures("tsne")}
        out = {"lda": self.embedding_figures("lda"),
               "plan": [self.plan_figures(p) for p in self.plan_patients]}
        if self.pairs_table is not None and self.pairs_root is not None:
            frame = read_pairs_table(self.pairs_table)
            z_pre = torch.cat([self._load_and_encode(os.path.join(str(self.pairs_root), n)) for n in frame["Pre name"]])
            z_post = torch.cat([self._load_and_encode(os.path.join(str(self.pairs_root), n))
                                for n in frame["Post name"]])
            out["prepost"] = self.prepost_figures(z_pre, z_post, list(frame["PID"]))
        return out

    # ------------------------------------------------------------ the whole run
    def _generator(self, step):
        return torch.Generator().manual_seed(self.seed + step)

    def metrics(self):
        """The quantitative part of :meth:`__call__`: writes and returns
        ``eval_metrics.json`` (``recon_errors`` ``{mean, median, max, std}``,
        ``train_set_diversity``, ``diversity``)."""
        out = {"recon_errors": self.reconstruction_errors(self._test_set),
               "train_set_diversity": self.compute_diversity_train_set(self._generator(3)),
               "diversity": self.compute_diversity(self.diversity_samples, self._generator(4))}
        _dump(self._path("eval_metrics.json"), out)
        return out

    STEPS = ("traversals", "embeddings", "classifiers", "generation", "metrics", "interpolate", "tsne", "plan",
             "prepost", "figures")
    # what the steps ``plan`` and ``prepost`` work on (``evaluate.py --patient / --pairs / --pairs-root``)
    plan_patients = ()
    pairs_table = pairs_root = None
    # mode -> what figures.embedding_figures returned: the base images the plan and pair figures are drawn on
    figure_bases = {}

    def run(self, step):
        """One step of the evaluation by name (``STEPS``); ``interpolate``,
        ``tsne``, ``plan``, ``prepost`` and ``figures`` (:meth:`all_figures`)
        are not part of :meth:`__call__`, as
        in the reference (whose ``__call__`` draws the LDA embedding only).
        ``plan`` runs :meth:`classify_and_project` and
        :meth:`interpolate_syndrome_to_normal` on every mesh of
        ``plan_patients``, ``prepost`` :meth:`evaluate_all_pre_post_pairs` on
        ``pairs_table`` under ``pairs_root``."""
        if step == "traversals":
            return self.latent_traversals(use_z_stats=False, animations=self.animations)
        if step == "embeddings":
            return self.embeddings()
        if step == "classifiers":
            return self.test_classifiers()
        if step == "generation":
            return (self.random_generation_and_rendering(n_samples=16, generator=self._generator(1)),
                    self.random_generation_and_save(n_samples=16, generator=self._generator(2)))
        if step == "metrics":
            return self.metrics()
        if step == "interpolate":
            return self.interpolate(animations=self.animations)
        if step == "tsne":
            return self.tsne_embeddings(generator=self._generator(5))
        if step == "plan":
            if not self.plan_patients:
                raise ValueError("the step 'plan' needs plan_patients (evaluate.py --patient PATH)")
            return [(self.classify_and_project(p), self.interpolate_syndrome_to_normal(p, animations=self.animations))
                    for p in self.plan_patients]
        if step == "prepost":
            if self.pairs_table is None or self.pairs_root is None:
                raise ValueError("the step 'prepost' needs pairs_table and pairs_root "
                                 "(evaluate.py --pairs FILE --pairs-root DIR)")
            return self.evaluate_all_pre_post_pairs(self.pairs_root, self.pairs_table)
        if step == "figures":
            return self.all_figures()
        raise ValueError(f"unknown step {step!r}; expected one of {self.STEPS}")

    def __call__(self):
        """``test.py:57-79``: 256-pixel renderings on white, the traversals
        (``use_z_stats=False``), with classifiers the embeddings and the
        classifier reports, random generation (picture and meshes), the three
        metrics -> ``eval_metrics.json``.  Returns the metrics."""
        self.set_renderings_size(256)
        self.set_rendering_background_color([1, 1, 1])
        self.run("traversals")
        if self.has_classifiers:
            self.run("embeddings")
            self.run("classifiers")
        self.run("generation")
        return self.run("metrics")


def evaluate_main(argv=None):
    """``evaluate.py`` (the reference's ``test.py:1443-1480``): read
    ``<output_path>/outputs/<id>/config.yaml``, resume the model and whatever
    classifier files its checkpoints folder holds, load the data sets and run
    the :class:`Tester` -- all of it, or the steps named by ``--only``.
    Returns the ``Tester``."""
    import argparse

    parser = argparse.ArgumentParser()
    parser.add_argument("--id", type=str, default="none", help="ID of experiment")
    parser.add_argument("--output_path", type=str, default=".", help="outputs path")
    parser.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--no-animations", action="store_true", help="write no animated PNG")
    parser.add_argument("--diversity-samples", type=int, default=10000, metavar="N",
                        help="latent pairs of the diversity figure")
    parser.add_argument("--only", default=None, metavar="NAME[,NAME]",
                        help="run only these steps: " + ", ".join(Tester.STEPS))
    parser.add_argument("--patient", action="append", default=[], metavar="PATH",
                        help="a patient's mesh file for the step 'plan' (may be given several times)")
    parser.add_argument("--pairs", default=None, metavar="FILE",
                        help="the table (.csv or .xlsx) of pre- / post-operative pairs for the step 'prepost'")
    parser.add_argument("--pairs-root", default=None, metavar="DIR", help="the folder of the meshes --pairs names")
    opts = parser.parse_args(argv)
    asked = [s for s in (opts.only or "").split(",") if s]
    if "plan" in asked and not opts.patient:
        parser.error("--only plan needs at least one --patient PATH")
    if "prepost" in asked and (opts.pairs is None or opts.pairs_root is None):
        parser.error("--only prepost needs --pairs FILE and --pairs-root DIR")

    from . import data as D
    from . import manager as M

    if not torch.cuda.is_available():
        raise RuntimeError("craniofacialsd_vae_amd evaluates on the GPU only (libcfsd); no GPU visible")
    output_directory = os.path.join(opts.output_path + "/outputs", opts.id)
    checkpoint_dir = os.path.join(output_directory, "checkpoints")
    config = M.load_config(os.path.join(output_directory, "config.yaml"))
    only = None
    if opts.only is not None:
        only = [s for s in opts.only.split(",") if s]
        bad = [s for s in only if s not in Tester.STEPS]
        if bad:
            parser.error(f"--only: unknown step(s) {bad}; expected {', '.join(Tester.STEPS)}")
    device = torch.device("cuda", torch.cuda.current_device())
    manager = M.ModelManager(config, device=device, precomputed_storage_path=config["data"]["precomputed_path"],
                             precision=opts.precision, seed=opts.seed, use_graph=False)
    manager.resume(checkpoint_dir)
    bs = config["optimization"]["batch_size"]
    train_set, _, test_set, norm = D.load_mesh_dataset(config["data"], bs, device, manager.template, seed=opts.seed)
    if test_set is None:
        raise ValueError(f"the test split holds fewer than one batch of {bs} meshes")
    tester = Tester(manager, norm if config["data"].get("normalize_data", True) else None, train_set, test_set,
                    output_directory, config, seed=opts.seed, animations=not opts.no_animations,
                    diversity_samples=opts.diversity_samples)
    tester.plan_patients, tester.pairs_table, tester.pairs_root = tuple(opts.patient), opts.pairs, opts.pairs_root
    if only is None:
        tester()
    else:
        tester.set_renderings_size(256)
        tester.set_rendering_background_color([1, 1, 1])
        for step in only:
            tester.run(step)
    return tester
