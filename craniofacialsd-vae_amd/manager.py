"""``ModelManager`` for the libcfsd training path: the reference's
orchestration (``model_manager.py:34-148`` construction, ``:176-238``
precompute / latent regions, ``:257-326`` run_epoch / _do_iteration,
``:575-592`` loss bookkeeping, ``:682-706`` checkpoints) driving
:class:`engine.SDVAEEngine` on resident data.

Differences by design (the reference's CPU loader and per-step host syncs are
what the MI355X path removes): batches come from :class:`engine.ResidentData`
(device-drawn epoch shuffle + on-device swap inside the step), the seven
``.item()`` per step become one device accumulator read per epoch, and the
train step can be replayed from a hipGraph.  ``render`` / ``log_images`` draw
with libcfsd's rasteriser (``rendering.py``) and write PNG files.  With a
``classifier:`` section the manager also carries the classifier stage
(``classify.ClassifierStage``: MLP, LDA, QDA and the region LDAs / QDAs,
``model_manager.py:403-573``) on libcfsd kernels -- with
``mlp_training_type: end2end`` the MLP is trained inside the VAE step
(``engine.SDVAEEngine.attach_classifier_head``); TensorBoard and the
``LinearSVC`` are out of scope.  The reference's
``Tester`` over a resumed manager is ``evaluation.Tester``.
"""
import json
import os

import numpy as np
import torch

from . import engine as E
from . import ops, precompute, refcache, topology
from .classify import ClassifierStage
from .step import TrainStep

LOSS_KEYS = ["reconstruction", "kl", "latent_consistency", "laplacian", "classification",
             "classification_acc", "tot"]


def load_config(path):
    """``utils.get_config`` (utils.py:64-66)."""
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def prepare_sub_folder(output_directory):
    """``utils.prepare_sub_folder`` (utils.py:69-74)."""
    d = os.path.join(output_directory, "checkpoints")
    os.makedirs(d, exist_ok=True)
    return d


def load_or_build_topology(config, template, precomputed_path):
    """The static geometry the model consumes (model_manager.py:176-230):
    ``topology.npz`` in ``precomputed_path`` (this package's cache), else the
    reference's own ``spirals.pkl`` + ``transforms.pkl`` (read without
    executing them), else built from the template by
    :func:`precompute.build_hierarchy` and cached.  Regions and Laplacian
    always come from the template (utils.py:77-144)."""
    os.makedirs(precomputed_path, exist_ok=True)
    cache = os.path.join(precomputed_path, "topology.npz")
    if os.path.exists(cache):
        return dict(np.load(cache))
    mp = config["model"]
    if os.path.exists(os.path.join(precomputed_path, "spirals.pkl")) and \
            os.path.exists(os.path.join(precomputed_path, "transforms.pkl")):
        h = refcache.load_precomputed(precomputed_path)
        h["pos_0"], h["face_0"] = template.pos, template.faces.astype(np.int32)
    else:
        h = precompute.build_hierarchy(template.pos, template.faces, template.colors,
                                       mp["sampling"]["sampling_factors"], mp["spirals"]["length"],
                                       mp["spirals"].get("dilation"), mp["sampling"].get("type", "basic"))
    if template.feat_and_cont is not None and "region_keys" not in h:  # (a fresh build wrote its own,
        keys = list(template.feat_and_cont.keys())                   # r_weighted-extended ones)
        h["region_keys"] = np.asarray(keys)
        for i, k in enumerate(keys):
            h[f"region_{i}_feature"] = np.asarray(template.feat_and_cont[k]["feature"], np.int32)
            h[f"region_{i}_contour"] = np.asarray(template.feat_and_cont[k]["contour"], np.int32)
    h["lap_row"], h["lap_col"], h["lap_val"] = template.laplacian
    np.savez(cache, **h)
    return h


def check_model_config(model_params):
    """Refuse, before any precompute, an architecture the kernels cannot run;
    the ``ValueError`` names the YAML key.  Any spiral length up to
    ``ops.GEN_MAX_SEQ`` and any channel count up to ``ops.GEN_MAX_CH`` trains
    (shapes without a specialised kernel take the general-shape ones); the
    hidden channel counts must be multiples of 4 (the Pool SpMM's rows)."""
    mp = model_params
    out_ch = [int(c) for c in mp["out_channels"]]
    if not out_ch:
        raise ValueError("model.out_channels is empty")
    for c in out_ch:
        if c < 4 or c % 4 or c > ops.GEN_MAX_CH:
            raise ValueError(f"model.out_channels {out_ch}: every entry must be a multiple of 4 in "
                             f"[4, {ops.GEN_MAX_CH}], got {c}")
    if not 1 <= int(mp["in_channels"]) <= ops.GEN_MAX_CH:
        raise ValueError(f"model.in_channels {mp['in_channels']} outside [1, {ops.GEN_MAX_CH}]")
    spirals = mp.get("spirals") or {}
    lengths = [int(n) for n in spirals.get("length", [])]
    for key, vals in (("length", lengths), ("dilation", spirals.get("dilation") or [])):
        if len(vals) and len(vals) != len(out_ch):
            raise ValueError(f"model.spirals.{key} has {len(vals)} entries, model.out_channels {len(out_ch)}")
    for n in lengths:
        if not 1 <= n <= ops.GEN_MAX_SEQ:
            raise ValueError(f"model.spirals.length {lengths}: every entry must lie in [1, {ops.GEN_MAX_SEQ}], got {n}")
    for d in spirals.get("dilation") or []:
        if int(d) < 1:
            raise ValueError(f"model.spirals.dilation {list(spirals['dilation'])}: every entry must be >= 1")


class JsonlWriter:
    """``SummaryWriter.add_scalar`` subset writing JSON lines (tensorboard is
    not installed in this image)."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, "scalars.jsonl")

    def add_scalar(self, tag, value, step):
        with open(self.path, "a") as f:
            f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")


class ModelManager(ClassifierStage):
    def __init__(self, configurations, device="cuda", precomputed_storage_path="precomputed",
                 precision="fp32", seed=0, use_graph=True, averager=None):
        self._model_params = configurations["model"]
        self._optimization_params = op = configurations["optimization"]
        self._precomputed_storage_path = precomputed_storage_path
        self._normalized_data = configurations["data"].get("normalize_data", True)
        self.to_mm_const = configurations["data"].get("to_mm_constant", 1.0)
        self.device = torch.device(device)
        self._swap_features = bool(configurations["data"].get("swap_features", True))
        if float(configurations["optimization"]["latent_consistency_weight"]) > 0 and not self._swap_features:
            # model_manager.py:93-94 (assert self._swap_features): the latent
            # consistency loss is defined on swapped bs x bs groups only
            raise ValueError("latent_consistency_weight > 0 needs data.swap_features: True")
        check_model_config(self._model_params)
        self.template = precompute.load_template(configurations["data"]["template_path"])
        self.topology_arrays = load_or_build_topology(configurations, self.template, precomputed_storage_path)
        self.topology = topology.DeviceTopology.from_npz(self.topology_arrays, device=self.device)
        self._w_latent_cons_loss = float(op["latent_consistency_weight"])
        self._w_laplacian_loss = float(op["laplacian_weight"])
        self._w_kl_loss = float(op["kl_weight"])
        mp = self._model_params
        spec = E.ModelSpec(mp["in_channels"], mp["out_channels"], mp["latent_size"],
                           is_vae=self._w_kl_loss > 0, pre_z_sigmoid=mp.get("pre_z_sigmoid", False))
        self.bs = int(op["batch_size"])
        self.engine = E.SDVAEEngine(
            self.topology, spec, lr=float(op["lr"]), weight_decay=float(op["weight_decay"]),
            w_kl=self._w_kl_loss, w_lc=self._w_latent_cons_loss, w_lap=self._w_laplacian_loss,
            eta1=float(op.get("latent_consistency_eta1", 0.5)), eta2=float(op.get("latent_consistency_eta2", 0.5)),
            swap_bs=self.bs, seed=seed, device=self.device, precision=precision,
            swap_features=self._swap_features)
        self._latent_regions = self._compute_latent_regions()
        self._init_classifiers(configurations, seed, end2end=True)  # nothing without a classifier: section
        # mlp_training_type: end2end -- the MLP's loss is a fifth term of the step (model_manager.py:295-318)
        self._w_classifier_loss = float(self._classifier_params["mlp_loss_weight"]) if self._mlp_end2end else 0.0
        self._batch_diagonal_idx = [(self.bs + 1) * i for i in range(self.bs)]
        self._losses = None
        self.use_graph = use_graph
        self._steps = {}
        # data-parallel (one process per GPU, train.py under torchrun): every
        # rank starts from rank 0's parameters and averages the gradient
        self.averager = averager
        if averager is not None and averager.world > 1:
            from .dist import broadcast_parameters
            broadcast_parameters(self.engine.params.data, 0)
            self.engine.sync_shadow()
            if self._mlp_end2end:  # the classifier is trained data-parallel too
                broadcast_parameters(self.classifier_mlp.flat, 0)
        self.val_acc = torch.zeros(6, dtype=torch.float32, device=self.device)
        self.val_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.val_cls_acc = torch.zeros(3, dtype=torch.float32, device=self.device)
        # what render() draws: the side of the square image and its background
        # (a grey level or an (r, g, b) triple); evaluation.Tester sets both
        self.renderings_size = 256
        self.renderings_background = 0.0

    # ------------------------------------------------------------ properties
    @property
    def loss_keys(self):
        return list(LOSS_KEYS)

    @property
    def latent_regions(self):
        return self._latent_regions

    @property
    def is_vae(self):
        return self._w_kl_loss > 0

    @property
    def batch_diagonal_idx(self):
        return self._batch_diagonal_idx

    def _compute_latent_regions(self):
        """model_manager.py:232-238: latent dims [i*size, (i+1)*size) per region."""
        names = list(self.template.feat_and_cont.keys())
        latent = self._model_params["latent_size"]
        assert latent % len(names) == 0
        size = latent // len(names)
        return {k: [i * size, (i + 1) * size] for i, k in enumerate(names)}

    # ------------------------------------------------------------ epochs
    def _train_step(self, b, data):
        """One training step from ``data`` through :class:`step.TrainStep`
        (the object bench.py times).  With ``use_graph`` the first step of a
        data set runs eagerly on a side stream and is captured; later steps
        replay the graph(s)."""
        ts = self._steps.get(id(data))
        if ts is None or ts.data is not data:
            ts = TrainStep(self.engine, data, self.averager, acc=self.engine.loss_acc)
            self._steps[id(data)] = ts
            if self.use_graph:
                ts.capture()  # includes one real (eager) step
                return "captured"
        ts.step()

    def _eval_step(self, b, data):
        """_do_iteration(train=False) (model_manager.py:274-326 under
        torch.no_grad(), eval mode: z = mu): the validation loader's shuffled,
        swapped batch on the device, forward + the four losses only."""
        eng, T = self.engine, self.topology
        ops.step_begin(self.val_counter, eng.seed + 7919, key=b.key, n_regions=max(T.n_regions, 1),
                       batch_idx=b.batch_idx, bs=self.bs, n_batches=data.n_batches, perm=data.rows,
                       n_items=data.n_items, shuffle=data.shuffle)
        eng.load_batch(b, data)
        eng.forward(b, train=False, acc=self.val_acc, finalize=True, cls_acc=self.val_cls_acc)

    def _prepare_end2end(self, data):
        """The classifier head of the step (``mlp_training_type: end2end``):
        attached once the class weights are known, and the data set's class
        indices put on the device.  The reference fails on its ``None``
        weights when ``set_class_conversions_and_weights`` has not run
        (``train.py:48`` calls it before the loop); so does this."""
        if self._class_weights is None:
            raise RuntimeError("mlp_training_type: end2end needs the class weights: call "
                               "set_class_conversions_and_weights(counts) before the first epoch")
        eng = self.engine
        if eng.head is None or eng.head.mlp is not self.classifier_mlp or eng.head.cw is not self._class_weights:
            eng.attach_classifier_head(self.classifier_mlp, self._class_weights, self._w_classifier_loss)
            self._steps = {}  # recorded steps hold the previous head's buffers
        if getattr(data, "class_idx", None) is None and not hasattr(data, "labels"):
            raise ValueError("mlp_training_type: end2end needs the data set's labels (ResidentData.labels, as "
                             "data.load_mesh_dataset sets them, or ResidentData.class_idx)")
        if hasattr(data, "labels") and (data.class_idx is None
                                        or getattr(data, "class2idx", None) != self._class2idx_dict):
            data.set_class_idx(self.class2idx([lab[0] for lab in data.labels]))
            data.class2idx = dict(self._class2idx_dict)

    def run_epoch(self, data, train=True, record=None):
        """``ModelManager.run_epoch`` (model_manager.py:257-272): every batch
        of one (shuffled, drop_last) epoch; returns and stores the per-batch
        mean of the losses (``_reset/_add/_divide_losses``).  ``record`` (a
        list) receives (batch_idx, key, eps) of every step (parity tests)."""
        b = self.engine.buffers(self.engine.step_rows)
        acc = self.engine.loss_acc if train else self.val_acc
        acc.zero_()
        cacc = self.engine.cls_acc if train else self.val_cls_acc
        if self._mlp_end2end:
            self._prepare_end2end(data)
            cacc.zero_()
        # writes made through ``net`` (a torch optimizer on its parameters,
        # net.load_state_dict) reach the fp32 master but not the bf16 shadow
        # the bf16 kernels read: refresh it once per epoch (one cast launch)
        self.engine.sync_shadow()
        steps_done = 0
        while steps_done < data.n_batches:
            if train:
                r = self._train_step(b, data)
                steps_done += 1
                if record is not None and r == "captured":
                    raise RuntimeError("record=... needs use_graph=False")
            else:
                self._eval_step(b, data)
                steps_done += 1
            if record is not None:
                record.append((b.batch_idx.cpu().numpy().copy(), int(b.key.item()),
                               b.eps.cpu().numpy().copy() if (train and self.is_vae) else None))
        if self.averager is not None and self.averager.world > 1:
            import torch.distributed as dist
            dist.all_reduce(acc)  # every rank's batches: sums and the batch count
            if self._mlp_end2end:
                dist.all_reduce(cacc)
        a = acc.cpu().numpy().astype(np.float64)
        if train:
            self.engine.check_health()  # a timed-out device wait invalidates the epoch: fail loudly
        n = max(a[5], 1.0)
        cls, cls_acc, tot = 0.0, 0.0, a[4] / n
        if self._mlp_end2end:  # the step's own total has the four VAE terms; the fifth is added here
            c = cacc.cpu().numpy().astype(np.float64)
            cls, cls_acc = c[0] / max(c[2], 1.0), c[1] / max(c[2], 1.0)
            tot = tot + self._w_classifier_loss * cls
        self._losses = {"reconstruction": a[0] / n, "kl": a[1] / n, "latent_consistency": a[2] / n,
                        "laplacian": a[3] / n, "classification": cls, "classification_acc": cls_acc,
                        "tot": tot}
        return dict(self._losses)

    def log_losses(self, writer, epoch, phase="train", losses=None):
        """model_manager.py:587-592 (``losses``: a run_epoch result; default
        the last one)."""
        losses = self._losses if losses is None else losses
        for k in self.loss_keys:
            writer.add_scalar(phase + "/" + str(k), losses[k], epoch + 1)

    # ------------------------------------------------------------ model access
    @property
    def net(self):
        """The drop-in :class:`model.Model` (``ModelManager._net``,
        ``model_manager.py:60-67``) over the engine's parameter STORAGE: its
        ``nn.Parameter``s are views of the flat buffer, so the engine's Adam
        updates are what it computes with.  Autograd runs through libcfsd
        (``model.py`` autograd Functions); parameter gradients it produces
        land in the module's own ``.grad`` tensors, not in the engine's.
        Read-mostly: a write through it (an optimizer step on its parameters,
        ``load_state_dict``) updates the fp32 master; in bf16 mode call
        :meth:`sync_from_net` afterwards (``run_epoch`` also refreshes the
        bf16 shadow at every epoch start)."""
        if getattr(self, "_net", None) is None:
            self._net = _engine_model(self.engine, self.topology_arrays, self._model_params, self.device)
        return self._net

    def sync_from_net(self):
        """Refresh the engine's bf16 weight shadow after writes made through
        :attr:`net` (no-op in fp32)."""
        self.engine.sync_shadow()

    def forward(self, data):
        """``ModelManager.forward`` (``model_manager.py:240-241``):
        ``self._net(data.x)`` in the module's current train / eval mode, with
        autograd.  ``data``: an object with ``.x`` [B, V, 3] (a ``Data``
        batch) or the tensor itself."""
        x = data.x if hasattr(data, "x") else data
        return self.net(x.to(self.device))

    def generate_for_opt(self, z):
        """``ModelManager.generate_for_opt`` (``model_manager.py:253-255``):
        decode in train mode WITH autograd, so a caller can optimise ``z``
        (the reference's latent fitting).  Returns [N, V, 3]."""
        self.net.train()
        return self.net.decode(z.to(self.device))

    def fit_mesh(self, verts, landmarks, landmark_idx, norm, latent_stats, faces=None, **kw):
        """``Tester.fit_mesh`` (``test.py:336-443``): fit the decoder to an
        unregistered scan.  ``verts`` ``[P, 3]`` the scan's vertices (any
        order), ``landmarks`` ``[L, 3]`` points on it, ``landmark_idx`` the
        ``L`` template vertices they correspond to, ``norm`` the ``norm.pt``
        dictionary (``mean`` / ``std``; None for un-normalised data),
        ``latent_stats`` the ``z_stats.pt`` dictionary (``means``).  The scan
        is aligned to the template (:func:`fitting.procrustes_align`), then
        :func:`fitting.fit_points` runs over :meth:`generate_for_opt`
        (``**kw``: its options).  ``faces`` ``[Fs, 3]`` (the scan's triangles,
        zero-based) switches the shape term to the distance between the
        SURFACES of the scan and of the decoded heads (the template's faces)
        and fills ``surface_mm``.  ``search="grid"`` (one of the options)
        searches the vertex path's nearest neighbours through uniform grids,
        for dense raw scans: the same result, bit for bit.  Returns
        ``(FitResult, aligned_verts)``;
        the result's errors, histories and ``surface_mm`` are multiplied by
        ``to_mm_const``."""
        from . import fitting
        if faces is not None:
            kw["target_faces"] = torch.as_tensor(np.asarray(faces, np.int64), dtype=torch.int32).to(self.device)
            kw["template_faces"] = torch.as_tensor(np.asarray(self.template.faces, np.int64),
                                                   dtype=torch.int32).to(self.device)
        lidx = np.asarray(landmark_idx, np.int64).reshape(-1)
        aligned, aligned_lnd = fitting.procrustes_align(landmarks, self.template.pos[lidx], verts)
        use_norm = norm is not None and self._normalized_data
        res = fitting.fit_points(
            self.generate_for_opt, torch.as_tensor(aligned, dtype=torch.float32).to(self.device),
            torch.as_tensor(aligned_lnd, dtype=torch.float32), lidx,
            norm["mean"] if use_norm else None, norm["std"] if use_norm else None,
            latent_stats["means"], module=self.net, **kw)
        for name in ("errors_shape", "errors_lnd", "chamfer_history", "landmark_history"):
            setattr(res, name, getattr(res, name) * self.to_mm_const)
        if res.surface_mm is not None:
            res.surface_mm = res.surface_mm * self.to_mm_const
        return res, aligned

    def encode(self, x):
        """Eval-mode latents of device meshes [N, V, 3] (model_manager.py:243-246)."""
        return self.engine.encode_all(x, batch_size=self.bs * self.bs)

    def generate(self, z):
        """Decoder output for latents [N, latent] (model_manager.py:248-251)."""
        outs = []
        for s in range(0, z.shape[0], self.bs * self.bs):
            zz = z[s:s + self.bs * self.bs].contiguous()
            b = self.engine.buffers(zz.shape[0])
            self.engine.decode(b, z=zz)
            outs.append(b.out.clone())
        return torch.cat(outs)

    def compute_vertex_errors(self, out, gt):
        """model_manager.py:395-400 (on device)."""
        return ops.vertex_errors(out.contiguous(), gt.contiguous(), to_mm=self.to_mm_const)

    # ------------------------------------------------------------ pictures
    @property
    def template_faces(self):
        """The template's triangles as the int32 device tensor the renderer takes."""
        if getattr(self, "_template_faces", None) is None:
            self._template_faces = torch.as_tensor(np.asarray(self.template.faces, np.int64),
                                                   dtype=torch.int32).to(self.device)
        return self._template_faces

    @torch.no_grad()
    def render(self, batched_verts, vertex_errors=None, error_max_scale=None):
        """``ModelManager.render`` (``model_manager.py:625-658``): the meshes
        ``batched_verts`` ``[B, V, 3]`` (un-normalised) seen from ``dist=2.5,
        elev=0, azim=15`` at ``renderings_size`` (256) squared over
        ``renderings_background`` (0.0), ``[B, 3, S, S]`` on the device.
        Without ``vertex_errors``: grey 0.5, Gouraud-shaded under a point
        light at (0, 0, 3).  With ``vertex_errors`` ``[B, V]``: their plasma
        colours over ``[0, error_max_scale]``, unshaded."""
        from . import rendering
        verts = batched_verts.detach().to(self.device, torch.float32).contiguous()
        if vertex_errors is None:
            return rendering.render(verts, self.template_faces, shading="gouraud", image_size=self.renderings_size,
                                    background=self.renderings_background)
        colors = rendering.errors_to_colors(vertex_errors.to(self.device), 0, error_max_scale)
        return rendering.render(verts, self.template_faces, colors, shading="none", image_size=self.renderings_size,
                                background=self.renderings_background)

    @torch.no_grad()
    def log_images(self, in_data, out_dir, epoch, normalization_dict=None, phase="train", error_max_scale=5):
        """``ModelManager.log_images`` (``model_manager.py:594-614``) with a
        directory in the writer's place: ground truth | reconstruction | error
        map of every mesh of ``in_data`` (``.x`` or the tensor, ``[B, V, 3]``),
        side by side, in a grid of ``batch_size`` columns (4 without
        ``swap_features``), written to ``<out_dir>/<phase>_<epoch + 1:08d>.png``.
        Returns the path."""
        from . import rendering
        x = (in_data.x if hasattr(in_data, "x") else in_data).to(self.device, torch.float32)
        self.net.eval()  # as after the reference's validation pass: z = mu
        out = self.forward(x)[0]
        if self._normalized_data:
            mean = normalization_dict["mean"].to(self.device, torch.float32)
            std = normalization_dict["std"].to(self.device, torch.float32)
            x, out = x * std + mean, out * std + mean
        errors = self.compute_vertex_errors(out, x)
        log = torch.cat([self.render(x), self.render(out), self.render(out, errors, error_max_scale)], dim=-1)
        grid = rendering.make_grid(log, nrow=self.bs if self._swap_features else 4, padding=10, pad_value=1.0)
        os.makedirs(out_dir, exist_ok=True)
        return rendering.save_png(os.path.join(out_dir, f"{phase}_{epoch + 1:08d}.png"), grid)

    def visualization_batch(self, data):
        """The meshes :meth:`log_images` draws for a resident set: its first
        ``batch_size`` meshes and, with ``swap_features``, their ``bs x bs``
        swap on region 0 (the reference keeps the first batch of each loader,
        train.py:45-46)."""
        idx = data.rows[:self.bs] if data.rows is not None else torch.arange(self.bs, device=self.device)
        idx = idx.to(torch.int32).contiguous()
        if not self._swap_features:
            return data.meshes.index_select(0, idx.long())
        key = torch.zeros(1, dtype=torch.int32, device=self.device)
        return ops.swap_features(data.meshes, idx, self.topology.region_mask, key, self.bs)

    def save_weights(self, checkpoint_dir, epoch):
        """``model_manager.py:682-688``: the model and its optimiser; with
        ``mlp_training_type: end2end`` also ``mlp_classifier.pt`` (the
        reference's format) and, beyond the reference, the classifier's Adam
        state (``mlp_classifier_optimizer.pt``), so that a resumed run
        continues bit for bit."""
        name = self.engine.save_weights(checkpoint_dir, epoch)
        if self._mlp_end2end:
            mlp = self.classifier_mlp
            torch.save({"model": {k: v.detach().cpu().clone() for k, v in mlp.state_dict().items()}},
                       os.path.join(checkpoint_dir, "mlp_classifier.pt"))
            torch.save({"exp_avg": mlp.exp_avg.cpu(), "exp_avg_sq": mlp.exp_avg_sq.cpu(), "step": mlp.step.cpu()},
                       os.path.join(checkpoint_dir, "mlp_classifier_optimizer.pt"))
        return name

    def resume(self, checkpoint_dir):
        """``ModelManager.resume`` (``model_manager.py:690-706``): the last
        model and the optimiser state; with a ``classifier:`` section also
        whatever classifier files the folder holds."""
        epoch = self.engine.resume(checkpoint_dir)
        if self._classifier_params is not None:
            self.resume_classifiers(checkpoint_dir)
            opt = os.path.join(checkpoint_dir, "mlp_classifier_optimizer.pt")
            if self._mlp_end2end and os.path.exists(opt):
                sd, mlp = torch.load(opt, map_location="cpu", weights_only=True), self.classifier_mlp
                mlp.exp_avg.copy_(sd["exp_avg"])
                mlp.exp_avg_sq.copy_(sd["exp_avg_sq"])
                mlp.step.copy_(sd["step"])
        return epoch


def _engine_model(engine, arrays, model_params, device):
    """A :class:`model.Model` built from the precomputed topology (int64
    spirals, sparse-COO transforms in file order, as the reference unpickles
    them) whose parameters are re-bound to views of ``engine.params.data``."""
    import torch.nn as nn

    from . import model as M
    n = int(arrays["n_levels"])
    spirals = [torch.from_numpy(np.asarray(arrays[f"spiral_{l}"], np.int64)).to(device) for l in range(n)]

    def sp(name, l):
        idx = np.stack([arrays[f"{name}_{l}_row"], arrays[f"{name}_{l}_col"]]).astype(np.int64)
        return torch.sparse_coo_tensor(torch.from_numpy(idx),
                                       torch.from_numpy(np.asarray(arrays[f"{name}_{l}_val"], np.float32)),
                                       tuple(np.asarray(arrays[f"{name}_{l}_shape"]).tolist()))

    S = engine.spec
    net = M.Model(S.in_ch, S.out_ch, S.latent, spirals, [sp("down", l) for l in range(n)],
                  [sp("up", l) for l in range(n)], pre_z_sigmoid=bool(model_params.get("pre_z_sigmoid", False)),
                  is_vae=S.is_vae).to(device)
    for name, _ in list(net.named_parameters()):
        *path, leaf = name.split(".")
        mod = net
        for p in path:
            mod = getattr(mod, p)
        setattr(mod, leaf, nn.Parameter(engine.params.view(name)))  # shares the flat buffer's storage
    return net
