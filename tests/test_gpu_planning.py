"""Surgical planning on the GPU (``csrc/planning.hip``, ``evaluation.py``;
reference ``test.py:652-1151``).

References.  ``plan_targets``: what scipy's ``multivariate_normal.logpdf`` gave
on the reference's 5000-point ``torch.linspace`` grid
(``tests/golden/make_planning.py`` -> ``planning_scipy.npz``), fed the golden's
float64 ``mean`` and ``whiten`` cast to fp32.  ``plan_tables``: the reference's
own composition, ``evaluation.vector_linspace`` plus slicing, on the CPU.
``pair_metrics``: ``scipy.spatial.distance`` on the float64 covariances (the
golden).  End to end: a float64 host evaluation of the grid under the manager's
own fitted parameters.

Bounds.  Distances: 1e-5 relative (fp32-stored parameters cost 6.5e-7, the
final fp32 rounding 6e-8; every sum is float64).  Indices: equal wherever the
reference's own crossing clears the level by more than 1e-5 of it (``margin``),
never more than one apart; at most 5 % of a case's crossings may be that close
(the reference alone: 2.0 %, 2.7 %, 0.7 %).  Grid points: ``4 * 2^-24 *
max(|s|, |e|)`` of ``torch.linspace``, whose vectorised CPU kernel a scalar
formula does not reproduce bit for bit (three roundings of relative size 2^-24
each side; the largest difference seen was 2.0 units).  ``dist``: ``(L + 3) *
2^-24`` relative of the float64 mean of the same fp32 table (the kernel sums in
float64 and rounds once: 2^-24).  Composed metrics against the golden: the
first-order propagation of 1e-5 per raw quantity, computed below.
"""
import json
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import classify_cases as cases
import recipe

pytestmark = pytest.mark.gpu
cfsd_loader.load()
from craniofacialsd_vae_amd import evaluation, ops  # noqa: E402
from test_evaluation_host import check_apng  # noqa: E402
from test_render_host import decode_png  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
LEVELS = (3.0, 2.0, 1.0)
STEPS = 5000
MARGIN = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planning_scipy.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def linspace_rows(z_row, mean, steps, rows):
    """Rows ``rows`` of ``vector_linspace(z_row, mean, steps)`` (CPU fp32)."""
    grid = evaluation.vector_linspace(z_row[None], mean[None], steps)
    return grid[torch.as_tensor(rows, dtype=torch.long)]


def host_crossings(z, mean, whiten, levels, steps):
    """Float64 evaluation of the reference's search on the CPU: per row of
    ``z`` (fp32 tensors; ``mean`` / ``whiten`` the fp32 parameters) the first
    point of the ``torch.linspace`` grid within each level, and its margin."""
    m64, w64 = mean.double().numpy(), whiten.double().numpy()
    index = np.empty((len(z), len(levels)), np.int64)
    margin = np.empty((len(z), len(levels)))
    for p in range(len(z)):
        grid = evaluation.vector_linspace(z[p][None], mean[None], steps).double().numpy()
        maha = np.sqrt((((grid - m64) @ w64) ** 2).sum(1))
        for k, level in enumerate(levels):
            i = int(np.argmax(maha <= level))
            index[p, k] = i
            margin[p, k] = min(level - maha[i], maha[i - 1] - level if i else np.inf) / level
    return index, margin


def check_indices(got, ref, margin, what, allowed=0.05):
    got, clear = got.cpu().numpy().astype(np.int64), margin > MARGIN
    excluded = 1.0 - clear.mean()
    print(f"{what}: {100 * excluded:.2f} % of {clear.size} crossings within the margin rule, "
          f"{int((got != ref).sum())} indices differ")
    assert excluded <= allowed, what
    assert np.array_equal(got[clear], ref[clear]), what
    assert np.abs(got - ref).max() <= 1, what


# ---------------------------------------------------------------- plan_targets
@pytest.mark.parametrize("name", ["full75", "region5", "odd20"])
def test_plan_targets_vs_golden(gold, name):
    case = cases.make_case(name)
    col0, d = case["cols"]
    z = torch.from_numpy(case["zt"])
    mean32 = torch.from_numpy(gold[f"{name}.mean"].astype(np.float32))
    maha, index, targets = ops.plan_targets(z.to(DEV), mean32.to(DEV), dev(gold[f"{name}.whiten"]), LEVELS, STEPS,
                                            cols=(col0, d))
    n = len(z)
    assert maha.shape == (n,) and index.shape == (n, 3) and index.dtype == torch.int32
    assert targets.shape == (n, 4, d) and targets.dtype == torch.float32
    ref = gold[f"{name}.maha"]
    err = np.abs(maha.cpu().double().numpy() - ref) / np.maximum(1.0, ref)
    print(f"{name}: distance {ref.min():.2f}..{ref.max():.2f}, largest error {err.max():.3e} (bound 1e-5)")
    assert err.max() <= 1e-5
    check_indices(index, gold[f"{name}.index"].astype(np.int64), gold[f"{name}.margin"], name)
    if name == "region5":  # patients already inside 3 sigma
        inside = ref <= 3.0 * (1 - MARGIN)
        assert inside.sum() >= 10 and bool((index[:, 0].cpu()[torch.from_numpy(inside)] == 0).all())
    # the targets are the grid points of the indices the kernel found
    idx, got, worst = index.cpu().numpy(), targets.cpu(), 0.0
    for p in range(n):
        zw = z[p, col0:col0 + d]
        want = linspace_rows(zw, mean32, STEPS, idx[p])
        unit = 4 * U * torch.maximum(zw.abs(), mean32.abs()).double()
        diff = (got[p, :3].double() - want.double()).abs()
        worst = max(worst, float((diff / (unit / 4)).max()))
        assert bool((diff <= unit).all()), (name, p)
    print(f"{name}: grid points at most {worst:.2f} x 2^-24 max(|s|, |e|) from torch.linspace (bound 4)")
    assert torch.equal(got[:, 3], mean32.expand(n, d))  # bit for bit


def _random_problem(n, d, seed, spread=2.0, ld=None, col0=0):
    g = torch.Generator().manual_seed(seed)
    ld = d if ld is None else ld
    mean = torch.randn(d, generator=g)
    q = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))[0]
    whiten = (q / torch.logspace(-0.5, 0.5, d, dtype=torch.float64)).float().contiguous()
    z = torch.randn(n, ld, generator=g) * spread
    z[:, col0:col0 + d] += mean
    return z.contiguous(), mean, whiten


@pytest.mark.parametrize("n,d,levels,steps", [
    (1, 75, LEVELS, STEPS), (7, 1, LEVELS, STEPS), (5, 128, LEVELS, STEPS), (6, 20, (2.5,), STEPS),
    (6, 20, (8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0), STEPS), (9, 20, LEVELS, 2), (4, 33, LEVELS, 3)])
def test_plan_targets_edge_rows(n, d, levels, steps):
    """n = 1, d = 1 and 128, one and eight levels, two steps (the patient or
    the mean) and three; in every case the first row IS the mean.  Against the
    float64 host search on the torch.linspace grid, under the rules of the
    golden cases."""
    z, mean, whiten = _random_problem(n, d, 100 * d + n + len(levels), ld=d + 3, col0=2)
    z[0, 2:2 + d] = mean
    if steps == 2:
        z[1, 2:2 + d] = mean + 0.01 * torch.randn(d, generator=torch.Generator().manual_seed(1))  # inside
    maha, index, targets = ops.plan_targets(z.to(DEV), mean.to(DEV), whiten.to(DEV), levels, steps, cols=(2, d))
    s = len(levels)
    assert index.shape == (n, s) and targets.shape == (n, s + 1, d)
    assert float(maha[0]) == 0.0 and bool((index[0] == 0).all())
    assert torch.equal(targets[0].cpu(), mean.expand(s + 1, d))
    ref, margin = host_crossings(z[:, 2:2 + d], mean, whiten, levels, steps)
    check_indices(index, ref, margin, f"n={n} d={d} S={s} steps={steps}")
    idx = index.cpu().numpy()
    assert (np.diff(idx, axis=1) >= 0).all() and idx.min() >= 0 and idx.max() <= steps - 1
    if steps == 2:
        assert set(np.unique(idx)) <= {0, 1} and bool((index[1] == 0).all()) and int(index[2:].min()) == 1
    assert torch.equal(targets[:, s].cpu(), mean.expand(n, d))


def test_plan_targets_is_deterministic_and_row_independent(gold):
    case = cases.make_case("full75")
    z = torch.from_numpy(case["zt"]).to(DEV)
    mean, whiten = dev(gold["full75.mean"]), dev(gold["full75.whiten"])
    first = ops.plan_targets(z, mean, whiten, LEVELS, STEPS)
    again = ops.plan_targets(z, mean, whiten, LEVELS, STEPS)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for p in (0, 100, 255):
        alone = ops.plan_targets(z[p:p + 1].contiguous(), mean, whiten, LEVELS, STEPS)
        assert all(torch.equal(a[0], b[p]) for a, b in zip(alone, first)), p


# ---------------------------------------------------------------- plan_tables
def _masks(n_procedures, latent, kind):
    mask = torch.zeros(n_procedures, latent, dtype=torch.uint8)
    if kind == "identity":  # one-column regions
        mask[torch.arange(n_procedures), torch.arange(n_procedures)] = 1
    elif kind == "overlap":  # windows of 15 columns every 6, the last procedure moves nothing
        for p in range(n_procedures - 1):
            mask[p, 6 * p:6 * p + 15] = 1
    elif kind == "tail":
        mask[:, latent // 2:] = 1
    return mask


@pytest.mark.parametrize("n_first", [1, 2, 8])
@pytest.mark.parametrize("n,latent,n_procedures,kind", [(1, 5, 0, None), (3, 20, 1, "tail"), (5, 75, 11, "overlap"),
                                                       (2, 15, 15, "identity")])
def test_plan_tables_vs_torch_composition(n, latent, n_procedures, kind, n_first):
    z, mean, whiten = _random_problem(n, latent, 7 * latent + n_first, spread=4.0)
    zd = z.to(DEV)
    _, index, targets = ops.plan_targets(zd, mean.to(DEV), whiten.to(DEV), LEVELS, STEPS)
    assert int(index.min()) > 0  # every path crosses every level on its way
    mask = _masks(n_procedures, latent, kind) if n_procedures else None
    tables, dist = ops.plan_tables(zd, targets, None if mask is None else mask.to(DEV), n_first)
    s, f, groups = 3, n_first + 3, 1 + n_procedures
    assert tables.shape == (n, groups, f, latent) and dist.shape == (n, groups, s + 1)
    got, tg = tables.cpu(), targets.cpu()
    worst = 0.0
    for p in range(n):
        for g in range(groups):
            moved = torch.ones(latent, dtype=torch.bool) if g == 0 else mask[g - 1].bool()
            want = z[p].repeat(f, 1)  # test.py:718-730
            if moved.any():
                want[:n_first, moved] = evaluation.vector_linspace(z[p:p + 1, moved], tg[p, :1, moved], n_first)
            for t in range(1, s + 1):
                want[n_first - 1 + t, moved] = tg[p, t, moved]
            assert torch.equal(got[p, g][:, ~moved], want[:, ~moved]), (p, g)       # kept columns: z, bit for bit
            assert torch.equal(got[p, g, n_first:], want[n_first:]), (p, g)          # copied targets
            assert torch.equal(got[p, g, 0], z[p]), (p, g)                           # a path starts at the patient
            unit = 4 * U * torch.maximum(z[p].abs(), tg[p, 0].abs()).double()
            diff = (got[p, g, :n_first].double() - want[:n_first].double()).abs()
            worst = max(worst, float((diff / (unit / 4)).max()))
            assert bool((diff <= unit).all()), (p, g)
            if not moved.any():
                assert torch.equal(got[p, g], z[p].expand(f, latent))               # an all-zero mask: z repeated
    ref = ((got[:, :, n_first - 1:].double() - tg[:, None, s:, :].double()) ** 2).mean(-1)
    err = ((dist.cpu().double() - ref).abs() / ref.clamp_min(1e-300)).max().item()
    print(f"n={n} L={latent} P={n_procedures} n_first={n_first}: linspace rows {worst:.2f} units (bound 4), "
          f"dist {err / U:.2f} x 2^-24 (bound {latent + 3})")
    assert bool(((dist.cpu().double() - ref).abs() <= (latent + 3) * U * ref).all())
    assert bool((dist[:, 0, s] == 0).all())  # the last row of group 0 IS the healthy mean
    if kind == "overlap":
        assert bool(mask[-1].sum() == 0) and bool((mask[:-1].sum(0) > 1).any())
    again = ops.plan_tables(zd, targets, None if mask is None else mask.to(DEV), n_first)
    assert torch.equal(again[0], tables) and torch.equal(again[1], dist)
    alone = ops.plan_tables(zd[-1:].contiguous(), targets[-1:].contiguous(), None if mask is None else mask.to(DEV),
                            n_first)
    assert torch.equal(alone[0][0], tables[-1]) and torch.equal(alone[1][0], dist[-1])


# ---------------------------------------------------------------- pair_metrics
N_PAIRS = 128


@pytest.fixture(scope="module")
def pairs(gold):
    zt = torch.from_numpy(cases.make_case("full75")["zt"])
    windows = [tuple(int(v) for v in w) for w in gold["pairs.windows"]]
    return {"pre": zt[:N_PAIRS].contiguous().to(DEV), "post": zt[N_PAIRS:2 * N_PAIRS].contiguous().to(DEV),
            "windows": windows, "mean": dev(gold["pairs.mean"]), "whiten": dev(gold["pairs.whiten"])}


@pytest.fixture(scope="module")
def raw(pairs):
    return ops.pair_metrics(pairs["pre"], pairs["post"], pairs["windows"], pairs["mean"], pairs["whiten"])


def test_pair_metrics_raw_vs_golden(gold, raw):
    assert raw.shape == (N_PAIRS, 16, 6) and raw.dtype == torch.float32
    got, ref = raw.cpu().double().numpy(), gold["pairs.raw"]
    for q, name in enumerate(ops.PAIR_RAW):
        scale = 1.0 if name == "cosine" else np.abs(ref[..., q])
        err = (np.abs(got[..., q] - ref[..., q]) / scale).max()
        print(f"{name}: largest error {err:.3e} ({'absolute' if name == 'cosine' else 'relative'}, bound 1e-5)")
        assert err <= 1e-5, name


def test_pair_metrics_composed(gold, raw):
    got, ref = raw.cpu().double().numpy(), gold["pairs.raw"]
    keys, affected = list(range(15)), [int(w) - 1 for w in gold["pairs.procedure_windows"]]
    out = [evaluation.compose_pair_metrics(got[i], keys, affected) for i in range(N_PAIRS)]
    # exactly the host formulas on the device's own raw values
    a, b, cos, length = got[..., 0], got[..., 1], got[..., 4], got[..., 5]
    distances, with_angle = (a - b) / b, length * cos / b
    l2 = (got[:, 0, 2] - got[:, 0, 3]) / got[:, 0, 3]
    for i, o in enumerate(out):
        assert o["global_metric"] == distances[i, 0] and o["global_metric_directional"] == with_angle[i, 0]
        assert o["global_metric_l2"] == l2[i]
        acc = 0.0
        for r in affected:
            assert o["region_metrics"][r] == {"metric_distances": distances[i, 1 + r],
                                              "metric_with_angle": with_angle[i, 1 + r]}
            acc += 1 * distances[i, 1 + r]
        assert o["procedure_metric"] == acc / len(affected) and sorted(o["region_metrics"]) == sorted(affected)
    # against the golden: each raw quantity carries 1e-5 (relative; the cosine absolute), to first order
    e = 1e-5
    ra, rb, rcos, rlen = ref[..., 0], ref[..., 1], ref[..., 4], ref[..., 5]
    tol_d = 2 * e * ra / rb                                  # d(a / b - 1)
    tol_a = 2 * e * np.abs(rlen * rcos / rb) + e * rlen / rb  # d(len cos / b)
    tol_l2 = 2 * e * ref[:, 0, 2] / ref[:, 0, 3]
    assert (np.abs(distances - gold["pairs.metric_distances"]) <= tol_d).all()
    assert (np.abs(with_angle - gold["pairs.metric_with_angle"]) <= tol_a).all()
    assert (np.abs(l2 - gold["pairs.global_metric_l2"]) <= tol_l2).all()
    proc = np.array([o["procedure_metric"] for o in out])
    rows = [1 + r for r in affected]
    assert (np.abs(proc - gold["pairs.procedure_metric"]) <= tol_d[:, rows].mean(1)).all()
    print(f"composed: metric_distances {np.abs(distances - gold['pairs.metric_distances']).max():.2e}, "
          f"metric_with_angle {np.abs(with_angle - gold['pairs.metric_with_angle']).max():.2e}")


def test_pair_metrics_zero_displacement_single_window_and_independence(pairs, raw):
    pre, post, windows = pairs["pre"], pairs["post"].clone(), pairs["windows"]
    post[5] = pre[5]
    got = ops.pair_metrics(pre, post, windows, pairs["mean"], pairs["whiten"])
    nan = torch.isnan(got)
    assert bool(nan[5, :, 4].all()) and int(nan.sum()) == len(windows)  # NaN in the cosines of that pair alone
    assert bool((got[5, :, 5] == 0).all()) and torch.equal(got[5, :, 0], got[5, :, 1])
    keep = [i for i in range(N_PAIRS) if i != 5]
    assert torch.equal(got[keep], raw[keep])
    assert torch.equal(ops.pair_metrics(pairs["pre"], pairs["post"], windows, pairs["mean"], pairs["whiten"]), raw)
    for w in (0, 1, 15):  # W = 1: a window alone, reading the same packed arrays
        alone = ops.pair_metrics(pairs["pre"], pairs["post"], [windows[w]], pairs["mean"], pairs["whiten"])
        assert alone.shape == (N_PAIRS, 1, 6) and torch.equal(alone[:, 0], raw[:, w])
    for p in (0, 77, 127):  # a pair alone
        alone = ops.pair_metrics(pairs["pre"][p:p + 1].contiguous(), pairs["post"][p:p + 1].contiguous(), windows,
                                 pairs["mean"], pairs["whiten"])
        assert torch.equal(alone[0], raw[p])


# ---------------------------------------------------------------- refusals
def test_wrappers_refuse_bad_arguments(pairs):
    z, mean, whiten = (t.to(DEV) for t in _random_problem(4, 20, 3))
    ok = ops.plan_targets(z, mean, whiten)
    for bad in (dict(z=z.double()), dict(z=z.cpu()), dict(mean=mean.cpu()), dict(whiten=whiten.half()),
                dict(mean=mean[:19].contiguous()), dict(cols=(5, 20)), dict(cols=(0, 0)), dict(levels=(1.0, 2.0, 3.0)),
                dict(levels=(2.0, 2.0)), dict(levels=(1.0, 0.0)), dict(levels=tuple(range(9, 0, -1))), dict(levels=()),
                dict(steps=1), dict(steps=2 ** 20 + 1), dict(z=z.t().contiguous().t())):
        args = {"z": z, "mean": mean, "whiten": whiten, **bad}
        with pytest.raises(ValueError):
            ops.plan_targets(args.pop("z"), args.pop("mean"), args.pop("whiten"), **args)
    targets = ok[2]
    mask = torch.ones(2, 20, dtype=torch.uint8, device=DEV)
    for bad in (dict(mask=torch.ones(2, 19, dtype=torch.uint8, device=DEV)), dict(mask=mask.bool()),
                dict(mask=mask.cpu()), dict(targets=targets[:3].contiguous()), dict(targets=targets.double()),
                dict(targets=targets[:, :, :19].contiguous()), dict(n_first=0), dict(n_first=65),
                dict(z=z.cpu())):
        args = {"z": z, "targets": targets, "mask": mask, **bad}
        with pytest.raises(ValueError):
            ops.plan_tables(args.pop("z"), args.pop("targets"), **args)
    pre, post, windows, pm, pw = pairs["pre"], pairs["post"], pairs["windows"], pairs["mean"], pairs["whiten"]
    for bad in (dict(z_pre=pre.double()), dict(z_post=post.cpu()), dict(z_post=post[:100].contiguous()),
                dict(windows=[(73, 5, 0, 0)]), dict(windows=[(0, 0, 0, 0)]), dict(windows=[(-1, 5, 0, 0)]),
                dict(windows=[(0, 5, pm.numel() - 4, 0)]), dict(windows=[(0, 5, 0, pw.numel() - 24)]),
                dict(windows=[]), dict(windows=[(0, 5, 0)]), dict(windows=[windows[1]] * 65), dict(mean=pm.cpu()),
                dict(whiten=pw.view(-1, 1))):
        args = {"z_pre": pre, "z_post": post, "windows": windows, "mean": pm, "whiten": pw, **bad}
        with pytest.raises(ValueError):
            ops.pair_metrics(**args)


# ---------------------------------------------------------------- end to end
TO_MM = 89.11
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
N_MESHES = 40


@pytest.fixture(scope="module")
def planner(tmp_path_factory, topo_npz):
    """A manager over the golden weights with a ``classifier:`` section, its
    QDA, LDA and region classifiers fitted (``.fit``, no training) on the
    encoded demo meshes -- the 12 golden meshes plus jittered copies, 40 files
    of the classes n / a / c / m --, three procedures made up for this test,
    and a Tester on the demo normalisation."""
    from craniofacialsd_vae_amd import manager as M
    from craniofacialsd_vae_amd import precompute
    d = tmp_path_factory.mktemp("demo_plan")
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    (d / "meshes").mkdir()
    m = recipe.load_meshes()
    rs = np.random.RandomState(3)
    names, verts = [], []
    for i in range(N_MESHES):
        v = (m["verts"][i % 12] + (0 if i < 12 else rs.normal(0, 0.002, m["verts"][0].shape))).astype(np.float32)
        names.append(f"{'nacm'[i % 4]}_{i:03d}.obj")
        verts.append(v)
        with open(d / "meshes" / names[-1], "w") as f:
            for p in v:
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": TO_MM,
                             "swap_features": True, "stratified_split": False})
    man = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"], use_graph=False)
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    norm = {"mean": torch.from_numpy(m["norm_mean"]).float().contiguous(),
            "std": torch.from_numpy(m["norm_std"]).float().contiguous()}
    x = (torch.from_numpy(np.stack(verts)) - norm["mean"]) / norm["std"]
    z = man.encode(x.to(DEV).contiguous()).contiguous()
    y = torch.tensor(man.class2idx([n[0] for n in names]), dtype=torch.int32)
    man.lda.fit(z, y, n_classes=4)
    man.qda.fit(z, y, n_classes=4)
    for key, (lo, hi) in man.latent_regions.items():
        man.region_ldas[key].fit(z, y, cols=(lo, hi - lo), n_classes=4)
        man.region_qdas[key].fit(z, y, cols=(lo, hi - lo), n_classes=4)
    keys = [str(k) for k in man.latent_regions]
    cfg["planning"] = {"procedures": {"front": [keys[0], keys[1]], "middle": [keys[1], keys[5], keys[6]],
                                      "last": [keys[14]]}}
    stats = {"means": torch.zeros(75), "stds": torch.ones(75), "mins": -torch.ones(75), "maxs": torch.ones(75)}
    tester = evaluation.Tester(man, norm, None, None, str(d / "out"), cfg, latent_stats=stats)
    return {"dir": d, "cfg": cfg, "manager": man, "tester": tester, "names": names, "z": z, "keys": keys}


def _png_size(path):
    w, h, _ = decode_png(str(path))
    return w, h


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_interpolate_syndrome_to_normal_end_to_end(planner):
    t, man, d = planner["tester"], planner["manager"], planner["dir"]
    patient = d / "meshes" / planner["names"][1]  # an 'a'
    out = t.interpolate_syndrome_to_normal(str(patient))
    assert man.renderings_size == 256 and man.renderings_background == 0.0  # put back
    groups, f = ["all_attributes", "front", "middle", "last"], evaluation.PLAN_FIRST + 3
    assert out["groups"] == groups and out["tables"].shape == (1, 4, f, 75) and out["dist"].shape == (1, 4, 4)
    # the crossings under the manager's own fitted parameters
    z = t._load_and_encode(str(patient))
    mean, whiten, cols = man.qda_gaussian("n")
    assert cols is None
    ref, margin = host_crossings(z.cpu(), mean.cpu(), whiten.cpu(), evaluation.PLAN_LEVELS, evaluation.PLAN_STEPS)
    print(f"patient at {float(out['maha'][0]):.4g}, crossings {out['index'][0].tolist()} (host {ref[0].tolist()}, "
          f"margins {margin[0].tolist()})")
    check_indices(out["index"], ref, margin, "end to end", allowed=1.0)
    assert int(out["index"][0, 0]) > 0  # (outside 3 sigma)
    # the decoded frames
    frames, errors = out["frames"], out["errors"]
    assert frames.shape == (4 * f, 17039, 3) and errors.shape == (4 * f, 17039)
    decoded = t._unnormalize_verts(t._decode(z))[0]
    for g in range(4):
        assert torch.equal(out["tables"][0, g, 0], z[0]) and torch.equal(frames[g * f], decoded), g
        assert bool((errors[g * f] == 0).all()) and bool((errors[g * f + f - 1] > 0).any())
    assert float(out["dist"][0, 0, 3]) == 0.0  # dm of moving everything
    assert bool((out["dist"][0, 1:, 3] > 0).all())
    lo, hi = man.latent_regions[list(man.latent_regions)[14]]
    assert torch.equal(out["tables"][0, 3, :, :lo], z[0, :lo].expand(f, lo))  # 'last' moves the last region only
    assert torch.equal(out["tables"][0, 3, -1, lo:hi], mean[lo:hi])
    # the files
    root = d / "out" / "interpolations"
    side = 512
    for name in groups:
        sub = root / f"a_001_{name}"
        assert _png_size(sub / f"a_001_{name}_interpolate.png") == (f * (side + 10) + 10, 2 * side + 20)
        shots = check_apng(str(sub / f"a_001_{name}_interpolate.apng"), f, fps=4)
        assert shots.shape[1:] == (side, 2 * side, 3) and bool((shots[0, 0, 0] == 255).all())  # on white
        for kind, colours in (("meshes", False), ("meshes_colormap", True)):
            assert sorted(os.listdir(sub / kind)) == sorted(f"{i}.ply" for i in range(f))
            head = open(sub / kind / "3.ply", "rb").read(300)
            assert b"element vertex 17039" in head and (b"property uchar red" in head) == colours
        emb = json.load(open(sub / "embedding.json"))
        assert np.asarray(emb["lda"]).shape == (f, 2) and list(emb["regions"]) == planner["keys"]
        assert all(np.asarray(v).shape == (f, 2) for v in emb["regions"].values())
    want = man.lda_project_latents_in_2d(out["tables"][0, 2])
    assert np.allclose(json.load(open(root / "a_001_middle" / "embedding.json"))["lda"], want.cpu().numpy())
    rows = open(root / "a_001_procedure_distances.csv").read().split()
    assert rows[0] == "procedure,d3,d2,d1,dm" and [r.split(",")[0] for r in rows[1:]] == groups[1:]
    for g, row in enumerate(rows[1:], start=1):
        assert [float(v) for v in row.split(",")[1:]] == out["dist"][0, g].cpu().double().tolist()
    # the patient alone, classified and projected
    point = t.classify_and_project(str(patient))
    assert point == json.load(open(root / "a_001_emb.json")) and point["class"] in "acmn"
    assert list(point["regions"]) == planner["keys"] and len(point["lda"]) == 2


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_pre_post_pairs_end_to_end(planner):
    t, man, d, names = planner["tester"], planner["manager"], planner["dir"], planner["names"]
    pairs_csv = d / "pairs.csv"
    rows = [("p1", names[1], names[4], "front", "monobloc", "Apert"), ("p2", names[2], names[8], "middle", "lefort", "Crouzon"),
            ("p3", names[13], names[16], "last", "monobloc", "Apert"), ("p4", names[3], names[3], "front", "lefort", "Muenke")]
    with open(pairs_csv, "w") as f:
        f.write(",".join(evaluation.PAIR_COLUMNS) + "\n" + "".join(",".join(r) + "\n" for r in rows))
    results = t.evaluate_all_pre_post_pairs(str(d / "meshes"), str(pairs_csv))
    out = d / "out" / "pre_post_eval"
    keys = planner["keys"]
    table = json.load(open(out / "region_metrics.json"))["rows"]
    import pandas as pd
    frame = pd.read_csv(out / "pairs_with_results.csv", dtype={"PID": str}, float_precision="round_trip")
    assert list(frame["PID"]) == ["p1", "p2", "p3", "p4"] and len(results) == len(table) == 4
    scalars = ("global_metric", "global_metric_l2", "global_metric_directional", "procedure_metric")
    affected = {"front": keys[:2], "middle": [keys[1], keys[5], keys[6]], "last": [keys[14]]}
    for i, (pid, pre, post, procedure, proc_name, syndrome) in enumerate(rows):
        stored = json.load(open(out / f"{pid}.json"))
        assert stored["patient_id"] == pid and stored["procedure"] == procedure
        assert list(stored["region_metrics"]) == affected[procedure] and np.asarray(stored["raw"]).shape == (16, 6)
        assert table[i]["Procedure"] == proc_name and table[i]["Syndrome"] == syndrome
        assert list(table[i]["metric_distances"]) == affected[procedure]
        assert abs(sum(stored["pre_posteriors"]) - 1) < 1e-12 and len(stored["pre_lda"]) == 2
        if i == 3:  # post == pre: the displacement is zero, its cosine undefined, everything else a number
            assert np.isnan(stored["global_metric_directional"]) and stored["global_metric"] == 0.0
            assert stored["global_metric_l2"] == 0.0 and stored["procedure_metric"] == 0.0
            assert stored["pre_class"] == stored["post_class"]
            continue
        assert all(np.isfinite(stored[k]) for k in scalars)
        assert [frame[k][i] for k in scalars] == [stored[k] for k in scalars]
        assert frame["pre_class"][i] == stored["pre_class"] and stored["pre_class"] in "acmn"
    # the same pairs one by one: the same numbers
    singles = [t.evaluate_pre_post_pair(str(d / "meshes" / pre), str(d / "meshes" / post), pid, procedure)
               for pid, pre, post, procedure, _, _ in rows[:3]]
    for one, many in zip(singles, results):
        for side in ("pre_lda", "post_lda"):  # (a torch matrix product: its bits may depend on the row count)
            assert np.allclose(one.pop(side), many.pop(side), rtol=1e-5, atol=1e-5)
        assert json.dumps(one, sort_keys=True) == json.dumps(many, sort_keys=True)
    # the whole latent's distances are the QDA's own
    ref = man.mahalanobis_dist_to_qda_distribution(
        torch.cat([t._load_and_encode(str(d / "meshes" / r[1])) for r in rows[:3]]))
    got = torch.tensor([r["raw"][0][0] for r in results[:3]], dtype=torch.float64)
    assert bool(((got - ref.cpu().double()).abs() <= 1e-4 * ref.cpu().double()).all())
    # with the region QDAs' accuracies present the procedure metric is weighted by them
    weights = {k: {"accuracy": 0.25 + 0.05 * r} for r, k in enumerate(keys)}
    with open(d / "out" / "classification_report_regions.json", "w") as f:
        json.dump(weights, f)
    weighted = t.evaluate_pre_post_pair(str(d / "meshes" / rows[1][1]), str(d / "meshes" / rows[1][2]), "p2", "middle")
    acc = 0.0
    for k in affected["middle"]:
        acc += weights[k]["accuracy"] * singles[1]["region_metrics"][k]["metric_distances"]
    assert weighted["procedure_metric"] == acc / 3 and weighted["procedure_metric"] != singles[1]["procedure_metric"]
    assert weighted["global_metric"] == singles[1]["global_metric"]
    os.remove(d / "out" / "classification_report_regions.json")
    # the post-operative colour map
    path = t.save_postop_colourmap(str(d / "meshes" / names[1]), str(d / "meshes" / names[4]))
    assert path.endswith("n_004_colmap.ply") and b"property uchar red" in open(path, "rb").read(300)
    with pytest.raises(ValueError, match="procedure"):
        t.evaluate_pre_post_pair(str(d / "meshes" / names[1]), str(d / "meshes" / names[4]), "p9", "unknown")
