"""The evaluation harness on the GPU (``csrc/evaluate.hip``, ``evaluation.py``;
reference ``test.py:57-334, 544-637, 1161-1419``).

References: ``ops.vertex_errors`` on the expanded first frames (bit for bit)
and ``oracle.vertex_errors`` for the group distances; the float64 mean of the
same fp32 device values for the region means; the CPU oracle's decoder
(``oracle.decode`` over the golden weights) for a traversal and for the
diversity core; for the whole run, the files it writes.

Bounds.  Group distances against the oracle: relative 1e-6, the tolerance
``test_vertex_errors_vs_oracle`` applies to the same arithmetic.  Region means:
``CFSD_RM_DEPTH(len) * 2^-24`` relative to the mean of ``|values|`` (every
term passes through at most ``depth`` roundings of relative size ``2^-24``; for
non-negative values that mean is the result itself).  Traversal against the
oracle: 1e-2 mm per vertex, 1e-3 mm for means, the tolerances of
``test_reconstruction_errors_c1`` for un-normalised errors and their means.
"""
import json
import os
import struct

import numpy as np
import pytest
import torch
import yaml

import cfsd_loader
import recipe
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu
cfsd_loader.load()
from craniofacialsd_vae_amd import evaluation, ops, topology  # noqa: E402
from test_evaluation_host import check_apng  # noqa: E402
from test_render_host import decode_png  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
TO_MM = 89.11


@pytest.fixture(scope="module")
def dtopo(topo_npz):
    return topology.DeviceTopology.from_npz(topo_npz, device=DEV)


# ---------------------------------------------------------------- group_vertex_errors
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("groups,n,nv", [(3, 4, 257), (1, 1, 1), (2, 10, 1300)])
def test_group_vertex_errors(groups, n, nv, normalise):
    """Bit-equal to cfsd_vertex_errors on the expanded first frames (which the
    kernel never sees), frame 0 of every group exactly 0, and within 1e-6 of
    the oracle."""
    g = torch.Generator().manual_seed(groups * 100 + n * 10 + nv)
    frames = torch.randn(groups * n, nv, 3, generator=g)
    mean = torch.randn(nv, 3, generator=g) if normalise else None
    std = torch.rand(nv, 3, generator=g) + 0.5 if normalise else None
    first = frames.view(groups, n, nv, 3)[:, :1].expand(groups, n, nv, 3).reshape(groups * n, nv, 3).contiguous()
    dev = (lambda t: None if t is None else t.to(DEV))
    got = ops.group_vertex_errors(frames.to(DEV), n, to_mm=TO_MM, mean=dev(mean), std=dev(std))
    want = ops.vertex_errors(frames.to(DEV), first.to(DEV), to_mm=TO_MM, mean=dev(mean), std=dev(std))
    assert got.shape == (groups * n, nv) and torch.equal(got, want)
    assert bool((got.view(groups, n, nv)[:, 0] == 0).all())
    ro, rf = (frames * std + mean, first * std + mean) if normalise else (frames, first)
    ref = O.vertex_errors(ro, rf, to_mm=TO_MM).double()
    err = (got.cpu().double() - ref).abs().max().item()
    print(f"groups {groups} n {n} nv {nv} normalise {normalise}: max err {err:.3e} of max {ref.max().item():.3e}")
    assert err <= 1e-6 * (1.0 + ref.abs().max().item())
    if n > 1:
        assert bool((got.view(groups, n, nv)[:, 1:] > 0).all())  # (random frames differ from their first)


def test_group_vertex_errors_refuses_bad_arguments():
    frames = torch.zeros(6, 5, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.group_vertex_errors(frames, 4)                  # 6 frames are no groups of 4
    with pytest.raises(ValueError):
        ops.group_vertex_errors(frames, 0)
    with pytest.raises(ValueError):
        ops.group_vertex_errors(frames[:, :, :2], 2)        # not [.., 3] (and not contiguous)
    with pytest.raises(ValueError):
        ops.group_vertex_errors(frames, 2, mean=torch.zeros(5, 3, device=DEV))  # std missing
    with pytest.raises(ValueError):
        ops.group_vertex_errors(frames.double(), 2)


# ---------------------------------------------------------------- region_means
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 513, 1300]


def _synthetic_regions(nv=1300, seed=2):
    """Unsorted lists of the lengths above; the two longest share vertices with
    every other list, and list 4 starts with the 100 entries list 5 ends with."""
    rs = np.random.RandomState(seed)
    lists = [rs.permutation(nv)[:n] for n in LENGTHS]
    lists[4][:100] = lists[5][-100:]
    assert len(set(lists[4]) & set(lists[5])) >= 100 and any(np.any(np.diff(lst) < 0) for lst in lists[1:])
    return lists


def _check_region_means(values, csr, what):
    got = ops.region_means(values, csr)
    assert got.shape == (values.shape[0], csr.n_regions) and got.dtype == torch.float32
    v64, idx = values.cpu().double(), csr.idx.cpu().long()
    signed = bool((values < 0).any())
    worst = 0.0
    for r in range(csr.n_regions):
        lst = idx[csr.ptr_host[r]:csr.ptr_host[r + 1]]
        ref = v64[:, lst].mean(1)
        scale = v64[:, lst].abs().mean(1) if signed else ref
        depth = ops.region_means_depth(len(lst))
        assert depth <= 32
        err = (got[:, r].cpu().double() - ref).abs()
        worst = max(worst, float((err / (depth * U * scale)).max()))
        assert bool((err <= depth * U * scale).all()), (what, r, len(lst))
    print(f"{what}: largest error {worst:.3f} of its bound")
    assert torch.equal(ops.region_means(values, csr), got)  # a second call: the same bits
    for b in (0, values.shape[0] - 1):                       # a row alone: the same bits
        assert torch.equal(ops.region_means(values[b:b + 1].contiguous(), csr)[0], got[b])
    return got


@pytest.mark.parametrize("signed", [False, True])
def test_region_means_synthetic(signed):
    nv = 1300
    csr = topology.RegionCSR(_synthetic_regions(nv), nv, device=DEV)
    g = torch.Generator().manual_seed(5 + signed)
    values = (torch.randn(5, nv, generator=g) if signed else torch.rand(5, nv, generator=g) * 7).to(DEV)
    got = _check_region_means(values, csr, f"synthetic signed={signed}")
    assert torch.equal(got[:, 0], values[:, int(csr.idx[0])])  # a list of one entry: the value itself


def test_region_means_template_regions(dtopo):
    """The 15 craniofacial regions on 17 039 vertices (the longest list: 3017)."""
    csr = dtopo.region_csr
    assert csr.n_regions == 15 and csr.nv == 17039 and max(csr.lengths) == 3017
    g = torch.Generator().manual_seed(8)
    _check_region_means((torch.rand(5, csr.nv, generator=g) * 5).to(DEV), csr, "template regions")
    _check_region_means(torch.randn(5, csr.nv, generator=g).to(DEV), csr, "template regions, mixed sign")
    # a constant map has that constant as every mean, exactly for a power of two
    assert bool((ops.region_means(torch.full((2, csr.nv), 0.25, device=DEV), csr) == 0.25).all())


def test_region_means_refuses_bad_arguments(dtopo):
    csr = dtopo.region_csr
    with pytest.raises(ValueError):
        ops.region_means(torch.zeros(2, 100, device=DEV), csr)          # another vertex count
    with pytest.raises(ValueError):
        ops.region_means(torch.zeros(csr.nv, device=DEV), csr)          # not [rows, V]
    with pytest.raises(ValueError):
        ops.region_means(torch.zeros(2, csr.nv, device=DEV).t().contiguous().t(), csr)  # not contiguous
    with pytest.raises(ValueError):
        ops.region_means(torch.zeros(2, 5, device=DEV), topology.RegionCSR([[0, 1]], 5, device="cpu"))


# ---------------------------------------------------------------- the demo workspace
CONFIG = {
    "optimization": {"epochs": 2, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
    "classifier": {"main_model_type": "qda", "mlp_training_type": "after", "mlp_hidden_features": [32, 16],
                   "mlp_lr": 1e-3, "mlp_epochs": 2},
    "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
}


@pytest.fixture(scope="module")
def workspace(tmp_path_factory, topo_npz):
    """The demo workspace: template, cached topology, 40 OBJ files of the
    classes n / a / c / m, and the configuration with a ``classifier:`` section."""
    from craniofacialsd_vae_amd import precompute
    d = tmp_path_factory.mktemp("demo_eval")
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    (d / "meshes").mkdir()
    m = recipe.load_meshes()
    rs = np.random.RandomState(3)
    for i in range(40):
        v = m["verts"][i % 12] + (0 if i < 12 else rs.normal(0, 0.002, m["verts"][0].shape))
        with open(d / "meshes" / f"{'nacm'[i % 4]}_{i:03d}.obj", "w") as f:
            for p in v.astype(np.float32):
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": TO_MM,
                             "swap_features": True, "stratified_split": False})
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return d, cfg


# ---------------------------------------------------------------- against the oracle's decoder
TRAVERSAL_LATENTS = [0, 74]
TRAVERSAL_STEPS = 3


@pytest.fixture(scope="module")
def golden(workspace, otopo, tmp_path_factory):
    """A manager over the golden weights with a Tester on the demo
    normalisation, and the oracle's decode of every latent the tests below
    use (six traversal frames, four diversity pairs), computed once."""
    from craniofacialsd_vae_amd import manager as M
    d, cfg = workspace
    cfg = {k: v for k, v in cfg.items() if k != "classifier"}
    man = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"], use_graph=False)
    w = recipe.golden_weights()
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = recipe.load_meshes()
    norm = {"mean": torch.from_numpy(m["norm_mean"]).float().contiguous(),
            "std": torch.from_numpy(m["norm_std"]).float().contiguous()}
    stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
    tester = evaluation.Tester(man, norm, None, None, str(tmp_path_factory.mktemp("golden_eval")), cfg,
                               latent_stats=stats)
    z_trav = tester.traversal_latents(use_z_stats=False, n_steps=TRAVERSAL_STEPS)[TRAVERSAL_LATENTS]
    g = torch.Generator().manual_seed(21)
    z_a, z_b = torch.randn(4, 75, generator=g), torch.randn(4, 75, generator=g)
    threads = torch.get_num_threads()  # (other modules pin the oracle's thread count: put it back)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        with torch.no_grad():
            dec = O.decode(O.make_params(w), torch.cat([z_trav.reshape(-1, 75), z_a, z_b]), otopo)
    finally:
        torch.set_num_threads(threads)
    dec = dec * norm["std"] + norm["mean"]
    n_t = len(TRAVERSAL_LATENTS) * TRAVERSAL_STEPS
    return {"tester": tester, "manager": man, "z_a": z_a, "z_b": z_b,
            "trav": dec[:n_t].view(len(TRAVERSAL_LATENTS), TRAVERSAL_STEPS, -1, 3), "a": dec[n_t:n_t + 4],
            "b": dec[n_t + 4:]}


def test_traversal_vs_oracle(golden, topo_npz):
    """latents 0 and 74 in three steps (-3, 0, 3): max_distances within 1e-2 mm
    per vertex of the oracle's decoder + compute_vertex_errors, the region table
    within 1e-3 mm of the reference's per-region torch.mean."""
    t = golden["tester"]
    out = t.latent_traversals(use_z_stats=False, latents=TRAVERSAL_LATENTS, n_steps=TRAVERSAL_STEPS, animations=False)
    ref = torch.stack([O.vertex_errors(f, f[0].expand(f.shape[0], -1, -1), to_mm=TO_MM)[-1] for f in golden["trav"]])
    got = out["max_distances"].cpu()
    err = (got - ref).abs().max().item()
    regions = [torch.from_numpy(topo_npz[f"region_{i}_feature"]).long() for i in range(15)]
    ref_table = torch.stack([torch.stack([torch.mean(row[r]) for r in regions]) for row in ref])
    err_t = (out["table"].cpu() - ref_table).abs().max().item()
    print(f"max_distances: max err {err:.3e} mm of max {ref.max().item():.2f} mm; table: max err {err_t:.3e} mm")
    assert got.shape == (2, 17039) and ref.max().item() > 1.0  # the traversal moves the head by millimetres
    assert err <= 1e-2
    assert out["table"].shape == (2, 15) and err_t <= 1e-3
    assert out["latents"] == TRAVERSAL_LATENTS and out["regions"] == [str(k) for k in topo_npz["region_keys"]]
    w, h = struct.unpack(">II", open(out["files"]["tiled"], "rb").read()[16:24])
    assert (w, h) == (2 * 266 + 10, 266 + 10)  # two 256-pixel maps in one row of the 5-column grid


def test_diversity_of_vs_oracle(golden):
    """Four injected pairs: within 1e-3 mm of the oracle; the per-pair figures
    and their mean do not depend on how the pairs are spread over calls."""
    t, z_a, z_b = golden["tester"], golden["z_a"], golden["z_b"]
    ref = torch.mean(O.vertex_errors(golden["a"], golden["b"], to_mm=TO_MM), dim=1)
    per_pair = t.pair_distances(z_a, z_b)
    got = t.diversity_of(z_a, z_b)
    print(f"diversity {got:.5f} mm, oracle {ref.mean().item():.5f} mm, per pair max err "
          f"{(per_pair.cpu() - ref).abs().max().item():.3e}")
    assert (per_pair.cpu() - ref).abs().max().item() <= 1e-3
    assert abs(got - ref.double().mean().item()) <= 1e-3
    halves = [t.pair_distances(z_a[s:s + 2], z_b[s:s + 2]) for s in (0, 2)]
    assert torch.equal(torch.cat(halves), per_pair)
    assert (t.diversity_of(z_a[:2], z_b[:2]) + t.diversity_of(z_a[2:], z_b[2:])) / 2 == got
    with pytest.raises(ValueError):
        t.diversity_of(z_a, z_b[:3])


# ---------------------------------------------------------------- end to end
def _png_size(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", raw[16:24])


@pytest.fixture(scope="module")
def evaluated(workspace):
    """2 epochs of training with the classifier stage through the driver, then
    the whole evaluation through ``evaluate_main``."""
    from craniofacialsd_vae_amd import train as T
    d, cfg = workspace
    T.main(["--config", str(d / "config.yaml"), "--id", "ev", "--output_path", str(d / "runs")])
    args = ["--id", "ev", "--output_path", str(d / "runs"), "--diversity-samples", "40", "--seed", "5"]
    tester = evaluation.evaluate_main(args)
    return d, cfg, tester, d / "runs" / "outputs" / "ev", args


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_evaluate_end_to_end(evaluated):
    d, cfg, tester, od, args = evaluated
    man = tester._manager
    assert man.renderings_size == 256 and man.renderings_background == (1.0, 1.0, 1.0)
    # the quantitative part
    metrics = json.load(open(od / "eval_metrics.json"))
    assert sorted(metrics) == ["diversity", "recon_errors", "train_set_diversity"]
    assert sorted(metrics["recon_errors"]) == ["max", "mean", "median", "std"]
    flat = list(metrics["recon_errors"].values()) + [metrics["diversity"], metrics["train_set_diversity"]]
    assert all(isinstance(v, float) and np.isfinite(v) and v > 0 for v in flat)
    # the whole traversal: 75 error maps, five per row
    assert _png_size(od / "latent_exploration_tiled.png") == (5 * 266 + 10, 15 * 266 + 10)
    table = json.load(open(od / "latent_exploration.json"))
    assert table["latents"] == list(range(75)) and np.asarray(table["mean_dist"]).shape == (75, 15)
    assert table["regions"] == [str(k) for k in man.topology.region_keys]
    for name, n_frames in (("latent_exploration.apng", 75 * (evaluation.N_STEPS + 2)),
                           ("latent_exploration_tiled.apng", evaluation.N_STEPS),
                           ("latent_exploration_out_tiled.apng", evaluation.N_STEPS)):
        head = open(od / name, "rb").read(64)  # signature, IHDR (25 bytes), then acTL: frames, plays
        assert head[37:41] == b"acTL" and struct.unpack(">II", head[41:49]) == (n_frames, 0), name
    # random generation
    assert _png_size(od / "random_generation.png") == (8 * 266 + 10, 2 * 266 + 10)
    assert sorted(os.listdir(od / "random_meshes")) == sorted(f"{i}.ply" for i in range(16))
    head = open(od / "random_meshes" / "0.ply", "rb").read(200)
    assert b"element vertex 17039" in head and f"element face {len(man.template.faces)}".encode() in head
    # three latent variables with the animations
    out = tester.latent_traversals(use_z_stats=False, latents=[0, 1, 2], animations=True)
    for key in ("tiled", "table", "animation", "tiled_animation", "out_tiled_animation"):
        assert os.path.exists(out["files"][key]), key
    assert _png_size(out["files"]["tiled"]) == (3 * 266 + 10, 266 + 10)
    frames = check_apng(out["files"]["animation"], 3 * (evaluation.N_STEPS + 2), fps=4)
    assert frames.shape[1:] == (256, 512, 3)
    assert not frames[10:12].any() and not frames[-2:].any() and frames[9].any()  # two black frames per latent
    assert bool((frames[0, 0, 0] == 255).all())  # white background
    tiled = check_apng(out["files"]["tiled_animation"], evaluation.N_STEPS, fps=1)
    out_tiled = check_apng(out["files"]["out_tiled_animation"], evaluation.N_STEPS, fps=4)
    assert tiled.shape == out_tiled.shape == (evaluation.N_STEPS, 276, 808, 3)
    _, _, last = decode_png(out["files"]["tiled"])  # the picture is the tiled animation's last frame
    assert np.array_equal(last, tiled[-1])
    again = json.load(open(out["files"]["table"]))
    assert again["latents"] == [0, 1, 2]
    want = ops.region_means(out["max_distances"], man.topology.region_csr)
    assert torch.equal(out["table"], want)
    assert np.array_equal(np.asarray(again["mean_dist"], np.float32), want.cpu().numpy())
    assert bool((out["max_distances"] > 0).any())
    # the classifier reports
    acc = json.load(open(od / "accuracies.json"))
    assert sorted(acc) == ["accuracy_lda", "accuracy_mlp", "accuracy_qda"]
    assert 0 <= acc["accuracy_mlp"] <= 100 and 0 <= acc["accuracy_lda"] <= 1 and 0 <= acc["accuracy_qda"] <= 1
    report = json.load(open(od / "classification_report.json"))
    assert sorted(report) == ["lda", "mlp", "qda"]
    for k in ("lda", "qda"):  # score() averages in fp32
        assert report[k]["accuracy"] == pytest.approx(acc[f"accuracy_{k}"], abs=1e-6)
        assert report[k]["weighted avg"]["support"] == tester._test_set.meshes.shape[0]
    cms = json.load(open(od / "confusion_matrices.json"))
    for k in ("mlp", "lda", "qda"):
        mat = np.asarray(cms[k]["matrix"])
        assert mat.shape == (len(cms[k]["labels"]),) * 2 and set(cms[k]["labels"]) <= set("acmn")
        assert all(s == pytest.approx(1.0) or s == 0.0 for s in mat.sum(1))
    regions = json.load(open(od / "classification_report_regions.json"))
    region_cms = json.load(open(od / "region_confusion_matrices.json"))
    assert list(regions) == [str(k) for k in man.latent_regions] and sorted(region_cms) == ["lda", "qda"]
    z = man.encode(tester._test_set.meshes)
    y = torch.tensor(man.class2idx([lab[0] for lab in tester._test_set.labels]))
    for key in man.latent_regions:
        assert regions[str(key)]["accuracy"] == man.region_qdas[key].score(z, y)
        assert list(region_cms["lda"]) == list(region_cms["qda"]) == list(regions)
    emb = np.load(od / "lda_embeddings.npz")
    n_tr, n_all = tester._train_set.meshes.shape[0], tester._train_set.meshes.shape[0] + len(z)
    assert emb["x1"].shape == emb["x2"].shape == emb["class"].shape == emb["is_test"].shape == (n_all,)
    assert emb["is_test"].sum() == len(z) and emb["augmented"].shape == (n_all,) and np.isfinite(emb["x1"]).all()
    assert all(emb[f"region_{i}"].shape == (n_tr, 2) for i in range(15))
    # interpolation between the two most different test meshes
    files = tester.interpolate()
    assert sorted(files) == ["all", "per_feature", "per_feature_animation", "per_variable_animation"]
    assert _png_size(files["all"]) == (15 * 266 + 10, 266 + 10)
    assert _png_size(files["per_feature"]) == (7 * 266 + 10, 15 * (266 + 10))
    check_apng(files["per_feature_animation"], 15 * 7, fps=4)
    check_apng(files["per_variable_animation"], 75 * 3, fps=4)
    # the same seed again, the metrics alone: the same file
    evaluation.evaluate_main(args + ["--only", "metrics"])
    assert json.load(open(od / "eval_metrics.json")) == metrics
