"""Fit the decoder to an unregistered scan: the reference's
``Tester.fit_mesh`` (``test.py:336-520``) on the libcfsd path.

Given a raw scan (vertices in any order, any pose and scale) and a handful of
landmarks on it, find the latent code whose decoded head matches the scan:

1. :func:`procrustes_align` -- the similarity alignment of the scan to the
   template through the landmarks (``test.py:350-373``), NumPy only;
2. :func:`fit_points` -- ``n_starts`` latent codes optimised together with
   Adam on ``10 * landmark MSE + Chamfer distance`` (``test.py:381-443``);
   the Chamfer term is :func:`ops.chamfer_distance` (HIP nearest-neighbour
   search; pytorch3d has no ROCm build) or, when the scan's and the
   template's faces are given, :func:`ops.surface_distance` (HIP
   point-to-triangle search: the distance to the SURFACES, free of the
   vertex-to-vertex term's sampling floor); ``search="grid"`` finds the
   Chamfer term's neighbours through exact uniform grids, for dense raw
   scans (bit-identical results); the decoder runs through
   ``model.py``'s autograd Functions with its parameters frozen, which
   selects their data-gradient-only backward;
3. :func:`fit_main` -- the ``fit.py`` command line.

Classifying the fitted latent (the QDA models), rendering and the plots of
the reference's method are out of scope.
"""
import contextlib
import json
from dataclasses import dataclass

import numpy as np
import torch

from . import ops


# ------------------------------------------------------------------ alignment
def procrustes_align(src_landmarks, dst_landmarks, src_points):
    """Similarity alignment of ``src_points`` ``[P, 3]`` onto the frame of
    ``dst_landmarks`` through corresponding landmarks ``[L, 3]``
    (``test.py:350-373``; ``dst`` = the template's landmarks, ``src`` = the
    scan's).

    Both landmark sets are centred and scaled to unit Frobenius norm (A from
    ``dst``, B from ``src``); ``R`` is the orthogonal matrix minimising
    ``|A R - B|_F`` (``scipy.linalg.orthogonal_procrustes``: ``R = U V^T`` of
    the SVD of ``A^T B``; REFLECTIONS ARE ALLOWED, det R may be -1, as in the
    reference's solver) and the scale is the sum of the singular values.
    Points and landmarks are mapped ``((p - c_src) / |B|) R^T * scale`` and
    back to the template's scale and centre.  float64 throughout.

    Returns ``(aligned_points [P, 3], aligned_landmarks [L, 3])``."""
    src = np.asarray(src_landmarks, np.float64)
    dst = np.asarray(dst_landmarks, np.float64)
    pts = np.asarray(src_points, np.float64)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape or len(src) < 3:
        raise ValueError(f"landmarks: shapes {src.shape} and {dst.shape}, expected two equal [L >= 3, 3] sets")
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"src_points: shape {pts.shape}, expected [P, 3]")
    c_dst, c_src = dst.mean(0), src.mean(0)
    a, b = dst - c_dst, src - c_src
    n_dst, n_src = np.linalg.norm(a), np.linalg.norm(b)
    if n_dst == 0 or n_src == 0:
        raise ValueError("landmarks: a landmark set is a single point")
    a, b = a / n_dst, b / n_src
    u, w, vt = np.linalg.svd(a.T @ b)
    rot, scale = u @ vt, w.sum()

    def to_dst(p):
        return (p @ rot.T) * scale * n_dst + c_dst

    return to_dst((pts - c_src) / n_src), to_dst(b)


# ------------------------------------------------------------------ the loop
@dataclass
class FitResult:
    """What :func:`fit_points` returns (device tensors; ``best`` a Python int)."""
    verts: torch.Tensor              # [V, 3] decoded vertices of the best start (un-normalised)
    z: torch.Tensor                  # [latent] the best start's latent after the last step
    z_all: torch.Tensor              # [n_starts, latent]
    z_init: torch.Tensor             # [n_starts, latent] the starts
    errors_shape: torch.Tensor       # [n_starts] Chamfer distance of each start's last decode
    errors_lnd: torch.Tensor         # [n_starts] landmark MSE of each start's last decode
    chamfer_history: torch.Tensor    # [iterations] the Chamfer term (mean over the starts)
    landmark_history: torch.Tensor   # [iterations] the landmark MSE (mean over the starts)
    best: int
    # with faces (the surface path): the mean UNSQUARED distance of the scan's vertices to the best fitted
    # head's surface, a 0-d device tensor; errors_shape and chamfer_history then hold the surface term
    surface_mm: torch.Tensor = None


@contextlib.contextmanager
def frozen(module):
    """Parameters of ``module`` with ``requires_grad`` False inside the block;
    the flags and every submodule's train / eval mode are put back exactly as
    found on exit (``module`` may be None)."""
    if module is None:
        yield
        return
    flags = [(p, p.requires_grad) for p in module.parameters()]
    modes = [(m, m.training) for m in module.modules()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        for m, t in modes:
            m.training = t


def fit_points(decode, target_points, target_landmarks, landmark_idx, mean, std, latent_mean, latent_std=None,
               n_starts=16, lr=5e-3, iterations=250, seed=0, selection_weights=(10.0, 1.0), landmark_weight=10.0,
               module=None, target_faces=None, template_faces=None, search="brute"):
    """The optimisation loop of ``Tester.fit_mesh`` (``test.py:381-443``).

    ``decode(z [n_starts, latent]) -> [n_starts, V, 3]`` with autograd (e.g.
    ``ModelManager.generate_for_opt``); ``target_points`` ``[P, 3]`` the
    aligned scan (any order, any P); ``target_landmarks`` ``[L, 3]`` its
    landmarks and ``landmark_idx`` the ``L`` template vertices they
    correspond to; ``mean`` / ``std`` ``[V, 3]`` un-normalise the decode
    (``gen * std + mean``; both None for un-normalised models).

    Starts: ``n_starts - 1`` standard-normal latents from a generator seeded
    with ``seed`` on the target's device (scaled and shifted by
    ``latent_std`` / ``latent_mean`` when ``latent_std`` is given; the
    reference draws plain ``randn``, the default) plus ``latent_mean``
    itself.  Every iteration: decode, un-normalise, loss = ``landmark_weight
    * MSE(gen[:, landmark_idx], landmarks) + chamfer_distance(gen, target)``,
    one ``torch.optim.Adam([z], lr)`` step.  Nothing is read back to the
    host inside the loop: both loss histories accumulate on the device.

    ``module`` (default: the ``nn.Module`` ``decode`` is bound to, if any):
    its parameters are frozen for the duration -- which makes ``model.py``'s
    autograd Functions skip every weight gradient -- and their
    ``requires_grad`` flags and the train / eval modes are restored in a
    ``finally``.

    ``target_faces`` ``[Fs, 3]`` (the scan's triangles) and ``template_faces``
    ``[F, 3]`` (the decoded heads'), device int32, given TOGETHER replace the
    Chamfer term by ``ops.surface_distance(gen, template_faces, target,
    target_faces)`` in the loss, in ``errors_shape`` and in the history, and
    fill ``surface_mm``; without them the loop is the vertex path unchanged.

    ``search``: how the Chamfer term finds its nearest neighbours.
    ``"brute"`` (the default) walks every pair; ``"grid"`` -- for DENSE raw
    scans, a few hundred thousand points and more -- searches uniform grids
    (``ops.PointGrid``): the grid over the scan is built once before the loop,
    the grids over the decoded heads every iteration, and every result is bit
    for bit that of ``"brute"``.  The surface term has its own culled search:
    ``search="grid"`` together with faces raises ``ValueError``.

    The best start is the argmin of ``w0 * errors_lnd + w1 * errors_shape``
    with ``selection_weights = (w0, w1)``.  The reference (``test.py:442``)
    computes ``10 * errors_lnd + errors_lnd``: the landmark error twice and
    the shape error never.  The default ``(10, 1)`` is the evident intent;
    ``selection_weights=(11, 0)`` reproduces the reference's choice.  As in
    the reference, the errors and the returned vertices are those of the
    last iteration's decode (before its Adam step), ``z`` is after it."""
    if n_starts < 1 or iterations < 1:
        raise ValueError("fit_points: n_starts and iterations must be >= 1")
    if (mean is None) != (std is None):
        raise ValueError("fit_points: mean and std go together")
    if module is None and isinstance(getattr(decode, "__self__", None), torch.nn.Module):
        module = decode.__self__
    if (target_faces is None) != (template_faces is None):
        raise ValueError("fit_points: target_faces and template_faces go together")
    if search not in ("brute", "grid"):
        raise ValueError(f'fit_points: search={search!r}, expected "brute" or "grid"')
    if search == "grid" and target_faces is not None:
        raise ValueError('fit_points: search="grid" is the vertex path\'s; the surface term (faces) has its own search')
    dev = target_points.device
    target = target_points.detach().to(torch.float32).reshape(1, -1, 3).contiguous()
    lnd = target_landmarks.detach().to(dev, torch.float32).reshape(1, -1, 3)
    lidx = torch.as_tensor(landmark_idx, dtype=torch.long, device=dev).reshape(-1)
    if lidx.numel() != lnd.shape[1]:
        raise ValueError(f"fit_points: {lidx.numel()} landmark indices for {lnd.shape[1]} landmarks")
    if mean is not None:
        mean, std = mean.detach().to(dev, torch.float32), std.detach().to(dev, torch.float32)
    latent_mean = latent_mean.detach().to(dev, torch.float32).reshape(-1)
    gen_rng = torch.Generator(device=dev)
    gen_rng.manual_seed(int(seed))
    starts = torch.randn((n_starts - 1, latent_mean.numel()), generator=gen_rng, device=dev, dtype=torch.float32)
    if latent_std is not None:
        starts = starts * latent_std.detach().to(dev, torch.float32).reshape(1, -1) + latent_mean
    z_init = torch.cat([starts, latent_mean[None]], 0)
    z = z_init.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr)
    ch_hist = torch.zeros(iterations, dtype=torch.float32, device=dev)
    lnd_hist = torch.zeros(iterations, dtype=torch.float32, device=dev)
    verts = None
    scan = None if target_faces is None else ops.SurfaceMesh(target, target_faces)
    if search == "grid":
        target = ops.PointGrid(target)  # built once: the scan is constant

    def shape_term(v, batch_reduction="mean"):
        if scan is None:
            return ops.chamfer_distance(v, target, batch_reduction=batch_reduction, search=search)[0]
        return ops.surface_distance(v, template_faces, scan, batch_reduction=batch_reduction)

    surface_mm = None
    with frozen(module):
        for it in range(iterations):
            opt.zero_grad()
            verts = decode(z)
            if mean is not None:
                verts = verts * std + mean
            lnd_loss = torch.mean((torch.index_select(verts, 1, lidx) - lnd) ** 2)
            ch_loss = shape_term(verts)
            (landmark_weight * lnd_loss + ch_loss).backward()
            opt.step()
            ch_hist[it] = ch_loss.detach()
            lnd_hist[it] = lnd_loss.detach()
        with torch.no_grad():
            verts = verts.detach()
            errors_shape = shape_term(verts, batch_reduction=None)
            errors_lnd = torch.mean(((verts[:, lidx, :] - lnd) ** 2).reshape(n_starts, -1), dim=1)
            w0, w1 = selection_weights
            best = int(torch.argmin(w0 * errors_lnd + w1 * errors_shape).item())  # the one host read
            if scan is not None:
                surface_mm = ops.point_mesh_distance(scan.queries, verts[best][None].contiguous(),
                                                     template_faces).sqrt().mean()
    z_all = z.detach()
    return FitResult(verts=verts[best], z=z_all[best], z_all=z_all, z_init=z_init, errors_shape=errors_shape,
                     errors_lnd=errors_lnd, chamfer_history=ch_hist, landmark_history=lnd_hist, best=best,
                     surface_mm=surface_mm)


# ------------------------------------------------------------------ command line
def read_landmarks(path):
    """The reference's landmark file: a JSON list of ``{"x", "y", "z"}``."""
    with open(path) as f:
        return np.asarray([[p["x"], p["y"], p["z"]] for p in json.load(f)], np.float64)


def fit_main(argv=None):
    """``fit.py``: fit a trained model to ``--mesh`` and write
    ``<out>_fit.obj`` (the fitted head, template faces), ``<out>_aligned.obj``
    (the aligned scan) and one JSON line with the errors (mm) and the best
    latent.  ``--surface`` reads the scan's faces too and fits to its
    triangles (:func:`ops.surface_distance`): the line then carries
    ``surface_mm`` and the aligned scan is written with its faces."""
    import argparse
    import os

    parser = argparse.ArgumentParser()
    parser.add_argument("--config", required=True, help="the training configuration (YAML)")
    parser.add_argument("--checkpoint-dir", required=True, help="folder holding model_%%08d.pt")
    parser.add_argument("--mesh", required=True, help="the scan (OBJ)")
    parser.add_argument("--landmarks", required=True, help="JSON list of {x, y, z} on the scan")
    parser.add_argument("--template-landmarks", required=True,
                        help="JSON list of the template vertex indices the landmarks correspond to")
    parser.add_argument("--z-stats", required=True, help="z_stats.pt written by train.py")
    parser.add_argument("--out", required=True, help="output prefix")
    parser.add_argument("--iterations", type=int, default=250)
    parser.add_argument("--lr", type=float, default=5e-3)
    parser.add_argument("--n-starts", type=int, default=16)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--surface", action="store_true",
                        help="fit to the scan's triangles (its f lines), not its vertices")
    parser.add_argument("--search", choices=("brute", "grid"), default="brute",
                        help="nearest-neighbour search of the Chamfer term: grid is for dense raw scans "
                             "(same result, bit for bit); not with --surface")
    parser.add_argument("--classifiers", default=None, metavar="CHECKPOINT_DIR",
                        help="folder holding the classifier files of train.py: also report the fit's class")
    opts = parser.parse_args(argv)
    if opts.surface and opts.search != "brute":
        parser.error("--search grid is the vertex path's; --surface has its own culled search")

    from . import data as D
    from . import manager as M

    if not torch.cuda.is_available():
        raise RuntimeError("craniofacialsd_vae_amd fits on the GPU only (libcfsd); no GPU visible")
    config = M.load_config(opts.config)
    manager = M.ModelManager(config, device="cuda", precomputed_storage_path=config["data"]["precomputed_path"],
                             use_graph=False)
    manager.resume(opts.checkpoint_dir)
    norm = None
    if config["data"].get("normalize_data", True):
        norm = torch.load(os.path.join(config["data"]["precomputed_path"], "norm.pt"), weights_only=True)
    with open(opts.template_landmarks) as f:
        landmark_idx = [int(i) for i in json.load(f)]
    scan = D.read_obj_vertices(opts.mesh)
    faces = None
    if opts.surface:
        faces = D.read_obj_faces(opts.mesh, n_verts=len(scan))
        if not len(faces):
            raise ValueError(f"--surface: {opts.mesh} has no faces")
    res, aligned = manager.fit_mesh(scan, read_landmarks(opts.landmarks), landmark_idx,
                                    norm, torch.load(opts.z_stats, weights_only=True), faces=faces, lr=opts.lr,
                                    iterations=opts.iterations, n_starts=opts.n_starts, seed=opts.seed,
                                    search=opts.search)
    D.write_obj(opts.out + "_fit.obj", res.verts.cpu().numpy(), manager.template.faces)
    D.write_obj(opts.out + "_aligned.obj", aligned, faces)
    shape_key = "surface_term_mm" if opts.surface else "chamfer_mm"
    line = {"best": res.best, shape_key: float(res.errors_shape[res.best]),
            "landmark_mm": float(res.errors_lnd[res.best]), "z": res.z.cpu().tolist()}
    if opts.surface:
        line["surface_mm"] = float(res.surface_mm)
    if opts.classifiers:  # test.py:446-451: encode the best fit, classify its latent with the QDA
        manager.resume_classifiers(opts.classifiers)
        v = res.verts.to(manager.device, torch.float32)
        if norm is not None:
            v = (v - norm["mean"].to(v.device)) / norm["std"].to(v.device)
        z_p = manager.encode(v.unsqueeze(0).contiguous())
        line["class_enc"] = manager.classify_latent(z_p, "qda")[0]
        if "n" in manager.class2idx_dict:
            line["maha_n"] = float(manager.mahalanobis_dist_to_qda_distribution(z_p, "n")[0])
    print(json.dumps(line))
    return line
