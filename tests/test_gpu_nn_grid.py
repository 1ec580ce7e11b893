"""The exact uniform-grid nearest-neighbour search (cfsd_nn_grid_build,
cfsd_nn_points_grid; ops.PointGrid, ops.nn_points_grid) and what is wired
through it: ops.chamfer_distance(search="grid"), fitting.fit_points and the
fit.py command line.

Oracle: the brute-force kernel, ops.nn_points, on the same tensors (itself
held to float64 by test_gpu_chamfer.py).  The grid search evaluates every
pair with the same instruction sequence and keeps the lexicographic minimum
of (distance bits, index), so the comparison is torch.equal on both outputs:
no tolerance anywhere in this file.
"""
import contextlib
import io
import json

import numpy as np
import pytest
import torch
import yaml

import cfsd_loader
import recipe
import synthetic_topology as ST

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import fitting, ops  # noqa: E402
from craniofacialsd_vae_amd import model as M  # noqa: E402

DEV = "cuda"
T = ops.NN_TILE


def _rand(shape, seed, scale=80.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _check(q, r, cells=None, stats=False):
    """nn_points_grid(q, PointGrid(r, cells)) against nn_points(q, r), bit for bit."""
    d0, i0 = ops.nn_points(q, r)
    out = ops.nn_points_grid(q, ops.PointGrid(r, cells), return_stats=stats)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[0].shape == d0.shape
    where = f"q {tuple(q.shape)} r {tuple(r.shape)} cells {cells}"
    assert torch.equal(out[1], i0), f"idx differs from brute force at {int((out[1] != i0).sum())} queries ({where})"
    assert torch.equal(out[0], d0), f"dist2 differs from brute force ({where})"
    if stats:
        p = r.shape[1]
        assert out[2].dtype == torch.int32 and out[2].shape == d0.shape
        assert int(out[2].min()) >= 1 and int(out[2].max()) <= p, f"counts outside [1, {p}] ({where})"
    return out


CELLS = [(1, 1, 1), (6, 6, 6), (1, 7, 128), None]


# ------------------------------------------------------------------ 1. shapes and broadcast forms
@pytest.mark.parametrize("bq,br", [(1, 1), (16, 16), (16, 1), (1, 16)])
def test_grid_matches_brute_force(bq, br):
    seed = 0
    for n in (1, 63, 65, 257):
        q = _rand((bq, n, 3), 100 + n)
        for p in (1, 15, 17, 300, 2000):
            seed += 1
            r = _rand((br, p, 3), 1000 + seed)
            for cells in CELLS:
                _check(q, r, cells, stats=True)


def test_point_set_forms():
    """[P, 3] is one set; a single set carries its Morton-ordered queries and
    a search FROM it returns the caller's order."""
    r = _rand((700, 3), 3)
    grid = ops.PointGrid(r, (5, 6, 7))
    assert grid.batch == 1 and grid.p == 700 and grid.points.shape == (1, 700, 3)
    assert torch.equal(grid.queries[0], r[grid.perm.long()])
    assert torch.equal(torch.sort(grid.perm).values, torch.arange(700, dtype=torch.int32, device=DEV))
    assert ops.PointGrid(_rand((2, 9, 3), 4)).perm is None
    other = ops.PointGrid(_rand((16, 300, 3), 5))
    d0, i0 = ops.nn_points(r[None], other.points)
    d1, i1 = ops.nn_points_grid(grid, other)  # Morton-ordered queries, results scattered back
    assert torch.equal(d1, d0) and torch.equal(i1, i0)
    assert ops.default_grid_cells(700) == ops.PointGrid(r).cells


# ------------------------------------------------------------------ 2. points on cell faces, ties across cells
def _lattice():
    a = torch.arange(5, dtype=torch.float32)
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(1, 125, 3).to(DEV)


def _half_queries():
    a = torch.arange(4, dtype=torch.float32) + 0.5
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(1, 64, 3).to(DEV)


def test_lattice_points_on_cell_faces():
    """5^3 integer lattice in (4, 4, 4) cells: every interior lattice plane IS
    a cell face; each half-integer query has 8 equidistant neighbours in
    several cells."""
    r, q = _lattice(), _half_queries()
    dist2, idx = _check(q, r, (4, 4, 4))[:2]
    assert bool((dist2 == 0.75).all())
    ref = ((q[0, :, None, :] - r[0, None, :, :]) ** 2).sum(-1)
    assert int((ref == 0.75).sum(1).min()) == 8
    for cells in ((3, 4, 5), (128, 128, 128), None):
        _check(q, r, cells)
    _check(r, r, (4, 4, 4))  # queries exactly on cell faces and corners


def test_duplicated_lattice_resolves_to_first_copy():
    r, q = _lattice().repeat(1, 2, 1), _half_queries()
    assert r.shape[1] == 250
    for cells in ((4, 4, 4), (7, 3, 2), None):
        _, idx = _check(q, r, cells)[:2]
        assert int(idx.max()) < 125


@pytest.mark.parametrize("p,period", [(40, 10), (300, 50)])
def test_repeated_points_resolve_to_lowest_index(p, period):
    base = _rand((1, period, 3), 5)
    r = base[:, torch.arange(p) % period].contiguous()
    q = _rand((3, 65, 3), 6)
    d0, i0 = ops.nn_points(q, base)
    for cells in ((6, 6, 6), (2, 9, 31), None):
        dist2, idx = _check(q, r, cells)[:2]
        assert int(idx.max()) < period
        assert torch.equal(idx, i0) and torch.equal(dist2, d0)


# ------------------------------------------------------------------ 3. far and sparse
def test_far_queries():
    r = _rand((2, 500, 3), 8, scale=1.0)
    q = _rand((2, 130, 3), 9, scale=1.0) + 1000.0
    for cells in ((6, 6, 6), (1, 7, 128), (32, 32, 32), None):
        _check(q, r, cells, stats=True)


def test_two_distant_blobs_many_empty_shells():
    a, b = _rand((1, 50, 3), 10, scale=0.3), _rand((1, 50, 3), 11, scale=0.3)
    b[..., 0] += 10.0
    r = torch.cat([a, b], 1)
    g = torch.Generator().manual_seed(12)
    q = torch.rand((1, 257, 3), generator=g).to(DEV) * torch.tensor([10.0, 0.6, 0.6], device=DEV)
    _, idx, count = _check(q, r, (16, 4, 4), stats=True)
    assert bool((idx < 50).any()) and bool((idx >= 50).any())
    _check(q, r, (128, 2, 2), stats=True)


# ------------------------------------------------------------------ 4. degenerate boxes
DEGENERATE_CELLS = [(1, 1, 1), (4, 4, 4), (1, 7, 128), (128, 128, 128), None]


@pytest.mark.parametrize("kind", ["coincident", "planar", "collinear", "single"])
def test_degenerate_boxes(kind):
    r = _rand((2, 200, 3), 13)
    if kind == "coincident":
        r[:] = torch.tensor([3.0, -7.0, 11.0], device=DEV)
    elif kind == "planar":
        r[..., 1] = 42.0
    elif kind == "collinear":
        r[..., 0], r[..., 2] = -5.0, 9.0
    else:
        r = r[:, :1].contiguous()
    q = torch.cat([_rand((2, 70, 3), 14), r[:, :3] + 0.0], 1).contiguous()
    for cells in DEGENERATE_CELLS:
        _, idx, _ = _check(q, r, cells, stats=True)
        if kind == "coincident":
            assert int(idx.max()) == 0  # 200 bit-equal candidates: the lowest index


# ------------------------------------------------------------------ 5. it culls
def test_grid_culls():
    """2048 points uniform on the unit sphere, 16^3 cells, queries just off the
    surface.  Cap: P / 16 = 128 points per query; a host restatement of the
    plain shell rule evaluates 12.3 on this very set (seed 5), ten times
    inside it (the kernel, which also skips rows inside a shell: 4.9)."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(2048, 3, generator=g)
    r = (v / v.norm(dim=1, keepdim=True)).float().to(DEV)[None].contiguous()
    q = (r[:, :200] * 1.01).contiguous()
    _, _, count = _check(q, r, (16, 16, 16), stats=True)
    mean = float(count.float().mean())
    print(f"points evaluated per query: mean {mean:.2f}, max {int(count.max())} of 2048")
    assert mean <= 2048 / 16


# ------------------------------------------------------------------ 6. chamfer
CHAMFER_CASES = {  # the shapes of test_gpu_chamfer.py's forward / backward test
    "shared_nearest": (2, 5, 300, 2),
    "broadcast_target": (3, 70, 40, 1),
    "odd": (4, 257, 2 * T + 3, 4),
}


@pytest.mark.parametrize("case", sorted(CHAMFER_CASES))
@pytest.mark.parametrize("batch_reduction", ["mean", "sum", None])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
def test_chamfer_grid_is_bit_identical(case, batch_reduction, point_reduction):
    bsz, n, p, by = CHAMFER_CASES[case]
    y = _rand((by, p, 3), 22 + p)
    upstream = None
    got = []
    for search, target in (("brute", y), ("grid", y), ("grid", ops.PointGrid(y)), ("grid", ops.PointGrid(y, (3, 5, 2)))):
        x = _rand((bsz, n, 3), 21 + n).requires_grad_(True)
        loss, none = ops.chamfer_distance(x, target, batch_reduction=batch_reduction,
                                          point_reduction=point_reduction, search=search)
        assert none is None
        if upstream is None:
            upstream = _rand(loss.shape, 23, scale=1.0) if batch_reduction is None else torch.tensor(1.7, device=DEV)
        (loss * upstream).sum().backward()
        got.append((loss.detach(), x.grad))
    for loss, grad in got[1:]:
        assert torch.equal(loss, got[0][0]) and torch.equal(grad, got[0][1])


def test_chamfer_grid_target_and_determinism():
    y = _rand((1, 700, 3), 32)
    grid = ops.PointGrid(y)
    outs = []
    for _ in range(2):
        x = _rand((4, 500, 3), 31).requires_grad_(True)
        loss, _ = ops.chamfer_distance(x, grid, batch_reduction=None, search="grid")
        loss.sum().backward()
        outs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError, match="PointGrid"):
        ops.chamfer_distance(_rand((4, 500, 3), 31), grid)  # a built grid is not brute force's operand
    with pytest.raises(ValueError, match="search="):
        ops.chamfer_distance(_rand((4, 500, 3), 31), y, search="tree")
    with pytest.raises(ValueError, match="must be 1 or"):
        ops.chamfer_distance(_rand((4, 50, 3), 31), ops.PointGrid(_rand((3, 20, 3), 1)), search="grid")


# ------------------------------------------------------------------ models for the fit tests
def _ref_inputs(npz):
    """What the reference passes to Model: int64 spirals + sparse COO transforms."""
    n = int(npz["n_levels"])
    spirals = [torch.from_numpy(np.asarray(npz[f"spiral_{l}"], np.int64)).to(DEV) for l in range(n)]

    def sp(name, l):
        idx = np.stack([npz[f"{name}_{l}_row"], npz[f"{name}_{l}_col"]]).astype(np.int64)
        return torch.sparse_coo_tensor(torch.from_numpy(idx),
                                       torch.from_numpy(np.asarray(npz[f"{name}_{l}_val"], np.float32)),
                                       tuple(np.asarray(npz[f"{name}_{l}_shape"]).tolist())).to(DEV)

    return spirals, [sp("down", l) for l in range(n)], [sp("up", l) for l in range(n)]


SMALL_CH, SMALL_LATENT = [32, 32, 64], 33
NU, NV = 24, 12


@pytest.fixture(scope="module")
def small():
    """The 288-vertex torus decoder and target of test_gpu_chamfer.py's fit test."""
    npz = ST.torus_topology(nu=NU, nv=NV, factors=(2, 2, 2))
    shapes = recipe.param_shapes(num_vert=36, out_ch=SMALL_CH, latent=SMALL_LATENT, is_vae=False)
    w = recipe.golden_weights(shapes, seed=4)
    spirals, down, up = _ref_inputs(npz)
    net = M.Model(3, SMALL_CH, SMALL_LATENT, spirals, down, up, is_vae=False).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    pos, _ = ST.torus_grid(NU, NV)
    mean = torch.from_numpy(pos.astype(np.float32))
    std = torch.from_numpy((0.05 + 0.02 * np.cos(np.arange(pos.size)).reshape(pos.shape)).astype(np.float32))
    g = torch.Generator().manual_seed(77)
    z_star = torch.randn(1, SMALL_LATENT, generator=g)
    lidx = [3, 61, 118, 176, 233]
    with torch.no_grad():
        full = (net.decode(z_star.to(DEV))[0].cpu() * std + mean)
    keep = torch.randperm(full.shape[0], generator=g)[:200]
    return net, mean, std, full[keep].contiguous(), full[lidx].contiguous(), lidx


FIT_FIELDS = ("z_all", "verts", "errors_shape", "errors_lnd", "chamfer_history", "landmark_history", "z_init", "z")


# ------------------------------------------------------------------ 7. fit
@pytest.mark.parametrize("permuted", [False, True])
def test_fit_points_grid_is_bit_identical(small, permuted):
    net, mean, std, target, lnd, lidx = small
    if permuted:  # the grid path's Morton order must not leak into the result
        target = target[torch.randperm(target.shape[0], generator=torch.Generator().manual_seed(9))].contiguous()
    res = {}
    for search in ("brute", "grid"):
        res[search] = fitting.fit_points(net.decode, target.to(DEV), lnd, lidx, mean, std, torch.zeros(SMALL_LATENT),
                                         n_starts=4, lr=5e-3, iterations=5, seed=0, search=search)
    for name in FIT_FIELDS:
        assert torch.equal(getattr(res["grid"], name), getattr(res["brute"], name)), name
    assert res["grid"].best == res["brute"].best
    assert (res["grid"].z_all - res["grid"].z_init).abs().max().item() > 1e-3  # the steps moved z


# ------------------------------------------------------------------ 8. command line
def _write_obj(path, v):
    with open(path, "w") as f:
        for p in v:
            f.write("v %.9g %.9g %.9g\n" % tuple(p))


def test_fit_cli_search_grid_writes_the_same_outputs(tmp_path, topo_npz):
    """fit.py's entry point on a demo workspace (golden weights saved as a
    checkpoint, demo mesh 5 with permuted vertices as the scan, a few
    iterations): --search grid writes what --search brute writes."""
    from craniofacialsd_vae_amd import manager as Mg
    from craniofacialsd_vae_amd import precompute
    d = tmp_path
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    meshes = recipe.load_meshes()
    torch.save({"mean": torch.from_numpy(meshes["norm_mean"]).float(), "std": torch.from_numpy(meshes["norm_std"]).float()},
               d / "pre" / "norm.pt")
    cfg = {
        "optimization": {"epochs": 1, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                         "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                         "latent_consistency_eta2": 0.5},
        "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
                  "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
                  "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
        "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
        "data": {"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                 "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": 89.11,
                 "swap_features": True, "stratified_split": False},
    }
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    man = Mg.ModelManager(cfg, device="cuda", precomputed_storage_path=cfg["data"]["precomputed_path"], seed=3,
                          use_graph=False)
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    (d / "ckpt").mkdir()
    man.save_weights(str(d / "ckpt"), 1)
    del man
    nv = meshes["verts"][5].shape[0]
    perm = np.random.RandomState(2).permutation(nv)
    scan = (meshes["verts"][5][perm] * 1.7 + np.array([5.0, -3.0, 2.0])).astype(np.float32)
    _write_obj(d / "scan.obj", scan)
    lidx = recipe.sample_idx(nv, k=12, seed=3).tolist()
    inv = np.empty(nv, np.int64)
    inv[perm] = np.arange(nv)
    with open(d / "lm.json", "w") as f:
        json.dump([dict(zip("xyz", map(float, scan[inv[i]]))) for i in lidx], f)
    with open(d / "idx.json", "w") as f:
        json.dump(lidx, f)
    torch.save({"means": torch.zeros(75), "stds": torch.ones(75)}, d / "z_stats.pt")
    base = ["--config", str(d / "config.yaml"), "--checkpoint-dir", str(d / "ckpt"), "--mesh", str(d / "scan.obj"),
            "--landmarks", str(d / "lm.json"), "--template-landmarks", str(d / "idx.json"), "--z-stats",
            str(d / "z_stats.pt"), "--iterations", "3", "--n-starts", "4", "--seed", "1"]
    lines = {}
    for search in ("brute", "grid"):
        with contextlib.redirect_stdout(io.StringIO()) as out:
            lines[search] = fitting.fit_main(base + ["--out", str(d / search), "--search", search])
        assert json.loads(out.getvalue().strip().splitlines()[-1]) == lines[search]
    assert lines["grid"] == lines["brute"] and "chamfer_mm" in lines["grid"]
    for suffix in ("_fit.obj", "_aligned.obj"):
        assert (d / ("grid" + suffix)).read_bytes() == (d / ("brute" + suffix)).read_bytes()
    assert (d / "grid_fit.obj").stat().st_size > 17039 * 10
    with pytest.raises(SystemExit):  # the surface term keeps its own search
        with contextlib.redirect_stderr(io.StringIO()):
            fitting.fit_main(base + ["--out", str(d / "s"), "--search", "grid", "--surface"])
