"""The Chamfer kernels (cfsd_nn_points, cfsd_chamfer_bwd), ops.chamfer_distance
and the latent fitting loop on the GPU.

Oracle: float64 brute force on the same fp32 inputs, inside this file.
Tolerances: the fp32 difference form (3 subtractions, 1 product, 2 fused
multiply-adds, no cancellation between the non-negative terms) is within
about 5 roundings of 2^-24 = 3e-7 of the exact value, so dist2 is held to
rtol 1e-6 and the returned index to d64(q, r[idx]) <= min_j d64 * (1 + 2e-6)
(tie-robust: no case is excluded).  Gradients are compared with float64
autograd of the same formula THROUGH THE KERNEL'S OWN INDICES (validated by
the nearest-neighbour tests), so the comparison is continuous through
near-ties: 1e-5 * (1 + max|ref|); losses rtol 1e-5.  The fit loop is held to
the project's step tolerance, 1e-4 relative.
"""
import numpy as np
import pytest
import torch

import cfsd_loader
import recipe
import synthetic_topology as ST
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import fitting, ops  # noqa: E402
from craniofacialsd_vae_amd import model as M  # noqa: E402

DEV = "cuda"
T = ops.NN_TILE


def _rand(shape, seed, scale=80.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _d64(q, r):
    """All squared distances in float64 by explicit differences, [B, N, P]."""
    q64, r64 = q.double(), r.double()
    return ((q64[:, :, None, :] - r64[:, None, :, :]) ** 2).sum(-1)


def _check_nn(q, r):
    dist2, idx = ops.nn_points(q, r)
    d = _d64(q, r)
    bsz, n, p = d.shape
    assert dist2.shape == (bsz, n) and idx.shape == (bsz, n)
    assert dist2.dtype == torch.float32 and idx.dtype == torch.int32
    assert int(idx.min()) >= 0 and int(idx.max()) < p
    dmin = d.min(-1).values
    rel = ((dist2.double() - dmin).abs() / dmin).max().item()
    assert rel <= 1e-6, f"dist2 rel err {rel:.3e} (B={bsz} N={n} P={p})"
    got = torch.gather(d, 2, idx.long()[:, :, None])[:, :, 0]
    assert bool((got <= dmin * (1 + 2e-6)).all()), f"a returned index is not a nearest point (B={bsz} N={n} P={p})"
    return dist2, idx


# ------------------------------------------------------------------ 1. NN vs float64
@pytest.mark.parametrize("bq,br", [(1, 1), (16, 16), (16, 1), (1, 16)])
def test_nn_points_matches_float64(bq, br):
    seed = 0
    for n in (1, 63, 65, 257):
        for p in (1, T - 1, T + 1, 2 * T + 3):
            seed += 1
            _check_nn(_rand((bq, n, 3), seed), _rand((br, p, 3), 1000 + seed))


@pytest.mark.parametrize("bq,br,n,p", [(1, 1, 65, 300), (2, 2, 600, 1000), (3, 1, 513, 257), (1, 4, 40, 129 * 3)])
def test_nn_points_cut_reference_range(bq, br, n, p):
    """Shapes whose reference range is cut into segments merged by the second
    launch (few queries, many reference points), all broadcast forms."""
    from craniofacialsd_vae_amd import _abi
    assert _abi.lib().cfsd_nn_points_workspace(max(bq, br), n, p) > 0
    _check_nn(_rand((bq, n, 3), 7 * n + p), _rand((br, p, 3), 11 * n + p))


# ------------------------------------------------------------------ 2. padding never wins
def test_nn_points_partial_chunk_has_no_phantom_point():
    """Queries near the origin, every reference point offset by +100 on every
    axis, P = T + 1: a padding point at the origin would win every query."""
    q = _rand((2, 65, 3), 1, scale=0.01)
    r = _rand((2, T + 1, 3), 2, scale=1.0) + 100.0
    dist2, idx = _check_nn(q, r)
    assert int(idx.max()) < T + 1
    assert float(dist2.min()) > 3 * 90.0 ** 2


# ------------------------------------------------------------------ 3. the last partial chunk is searched
@pytest.mark.parametrize("p", [T + 1, 2 * T + 3, 300])
def test_nn_points_neighbour_in_last_partial_chunk(p):
    q = _rand((2, 70, 3), 3, scale=0.01)
    r = _rand((1, p, 3), 4, scale=1.0) + 50.0
    r[:, p - 1] = 0.0
    _, idx = _check_nn(q, r)
    assert bool((idx == p - 1).all())


# ------------------------------------------------------------------ 4. ties -> lowest index
@pytest.mark.parametrize("p,period", [(40, 10), (300, 50)])
def test_nn_points_ties_resolve_to_lowest_index(p, period):
    """r[j] = base[j % period]: every point exists p / period times, in full
    chunks, in the partial last chunk and (p = 300) in both segments of a cut
    reference range.  Each query must get the FIRST copy of its nearest."""
    base = _rand((1, period, 3), 5)
    r = base[:, torch.arange(p) % period].contiguous()
    q = _rand((3, 65, 3), 6)
    dist2, idx = _check_nn(q, r)
    assert int(idx.max()) < period
    d0, i0 = ops.nn_points(q, base)
    assert torch.equal(idx, i0) and torch.equal(dist2, d0)


# ------------------------------------------------------------------ 5. chamfer forward / backward
def _chamfer_ref(x, y, idx_xy, idx_yx, batch_reduction, point_reduction, upstream):
    """float64 autograd of the Chamfer formula through fixed indices."""
    x64 = x.double().requires_grad_(True)
    y64 = y.double().expand(x.shape[0], -1, -1)
    near_y = torch.gather(y64, 1, idx_xy.long()[:, :, None].expand(-1, -1, 3))
    near_x = torch.gather(x64, 1, idx_yx.long()[:, :, None].expand(-1, -1, 3))
    cx, cy = ((x64 - near_y) ** 2).sum(-1), ((y64 - near_x) ** 2).sum(-1)
    per = (cx.mean(1) + cy.mean(1)) if point_reduction == "mean" else (cx.sum(1) + cy.sum(1))
    loss = per.mean() if batch_reduction == "mean" else per.sum() if batch_reduction == "sum" else per
    (loss * upstream.double()).sum().backward()
    return loss.detach(), x64.grad


CHAMFER_CASES = {
    "shared_nearest": (2, 5, 300, 2),      # many targets per generated point: long segments
    "broadcast_target": (3, 70, 40, 1),
    "odd": (4, 257, 2 * T + 3, 4),
}


@pytest.mark.parametrize("case", sorted(CHAMFER_CASES))
@pytest.mark.parametrize("batch_reduction", ["mean", "sum", None])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
def test_chamfer_distance_forward_backward(case, batch_reduction, point_reduction):
    bsz, n, p, by = CHAMFER_CASES[case]
    x = _rand((bsz, n, 3), 21 + n).requires_grad_(True)
    y = _rand((by, p, 3), 22 + p)
    loss, none = ops.chamfer_distance(x, y, batch_reduction=batch_reduction, point_reduction=point_reduction)
    assert none is None
    assert loss.shape == ((bsz,) if batch_reduction is None else ())
    upstream = _rand(loss.shape, 23, scale=1.0) if batch_reduction is None else torch.tensor(1.7, device=DEV)
    (loss * upstream).sum().backward()
    _, idx_xy = ops.nn_points(x.detach(), y)
    _, idx_yx = ops.nn_points(y, x.detach())
    if case == "shared_nearest":
        assert int(torch.bincount(idx_yx[0].long(), minlength=n).max()) > 20
    ref_loss, ref_grad = _chamfer_ref(x.detach(), y, idx_xy, idx_yx, batch_reduction, point_reduction, upstream)
    rel = ((loss.detach().double() - ref_loss).abs() / ref_loss.abs()).max().item()
    assert rel <= 1e-5, f"loss rel err {rel:.3e}"
    err, tol = (x.grad.double() - ref_grad).abs().max().item(), 1e-5 * (1 + ref_grad.abs().max().item())
    assert err <= tol, f"grad err {err:.3e} > {tol:.3e}"


def test_chamfer_backward_empty_segment():
    """A generated point that is nobody's nearest: only its own term remains."""
    x = torch.tensor([[[0.0, 0, 0], [10, 0, 0], [0, 10, 0], [500, 500, 500]]], device=DEV).requires_grad_(True)
    y = torch.tensor([[[1.0, 1, 0], [9, 1, 1], [1, 9, 2], [-1, 0, 1], [11, -1, 0], [0, 11, 1]]], device=DEV)
    _, idx_yx = ops.nn_points(y, x.detach())
    _, idx_xy = ops.nn_points(x.detach(), y)
    assert 3 not in idx_yx.tolist()[0]
    loss, _ = ops.chamfer_distance(x, y)
    loss.backward()
    one = torch.ones((), device=DEV)
    ref_loss, ref_grad = _chamfer_ref(x.detach(), y, idx_xy, idx_yx, "mean", "mean", one)
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * ref_loss.item()
    assert (x.grad.double() - ref_grad).abs().max().item() <= 1e-5 * (1 + ref_grad.abs().max().item())
    k = idx_xy[0, 3].long()
    expect = 2 * (x.detach()[0, 3] - y[0, k]).double() / 4
    assert (x.grad[0, 3].double() - expect).abs().max().item() <= 1e-5 * (1 + expect.abs().max().item())


def test_chamfer_target_is_constant():
    x, y = _rand((1, 4, 3), 1), _rand((1, 4, 3), 2).requires_grad_(True)
    with pytest.raises(ValueError):
        ops.chamfer_distance(x, y)


# ------------------------------------------------------------------ 6. determinism
def test_chamfer_bitwise_deterministic():
    outs = []
    for _ in range(2):
        x = _rand((4, 500, 3), 31).requires_grad_(True)
        y = _rand((1, 700, 3), 32)
        loss, _ = ops.chamfer_distance(x, y, batch_reduction=None)
        loss.sum().backward()
        outs.append((loss.detach().clone(), x.grad.clone(), *ops.nn_points(y, x.detach())))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


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
    """The 288-vertex torus (levels 288 / 144 / 72 / 36), AE, golden weights."""
    npz = ST.torus_topology(nu=NU, nv=NV, factors=(2, 2, 2))
    shapes = recipe.param_shapes(num_vert=36, out_ch=SMALL_CH, latent=SMALL_LATENT, is_vae=False)
    w = recipe.golden_weights(shapes, seed=4)
    spirals, down, up = _ref_inputs(npz)
    net = M.Model(3, SMALL_CH, SMALL_LATENT, spirals, down, up, is_vae=False).to(DEV)
    assert list(net.state_dict().keys()) == list(w.keys())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return net, w, O.Topology(npz)


def _pair_sq(a, b):
    return ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)


# ------------------------------------------------------------------ 7. fit loop vs host mirror
# The starts come from a DEVICE generator, so the mirror takes them from the
# result (z_init) and the near-tie condition below is asserted where the test
# runs; seed 0 satisfies it (smallest relative gap between a query's best and
# second-best squared distance over the 3 iterations: above 1e-5).
FIT_SEED = 0


def test_fit_points_matches_host_mirror(small):
    net, w, topo = small
    n_starts, iters, lr = 4, 3, 5e-3
    pos, _ = ST.torus_grid(NU, NV)
    mean = torch.from_numpy(pos.astype(np.float32))
    std = torch.from_numpy((0.05 + 0.02 * np.cos(np.arange(pos.size)).reshape(pos.shape)).astype(np.float32))
    g = torch.Generator().manual_seed(77)
    z_star = torch.randn(1, SMALL_LATENT, generator=g)
    lidx = [3, 61, 118, 176, 233]
    with torch.no_grad():
        full = (net.decode(z_star.to(DEV))[0].cpu() * std + mean)
    keep = torch.randperm(full.shape[0], generator=g)[:200]
    target, lnd = full[keep].contiguous(), full[lidx].contiguous()

    res = fitting.fit_points(net.decode, target.to(DEV), lnd, lidx, mean, std, torch.zeros(SMALL_LATENT),
                             n_starts=n_starts, lr=lr, iterations=iters, seed=FIT_SEED)
    assert res.z_all.shape == (n_starts, SMALL_LATENT) and res.verts.shape == (288, 3)
    assert torch.equal(res.z_init[-1].cpu(), torch.zeros(SMALL_LATENT))
    assert 0 <= res.best < n_starts and torch.equal(res.z, res.z_all[res.best])

    # host mirror: oracle decoder (fp32), Chamfer + landmark loss in float64, plain Adam
    P = {k: v.detach() for k, v in O.make_params(w).items()}
    z = {"z": res.z_init.cpu().clone().requires_grad_(True)}
    opt = O.Adam(z, lr=lr)
    t64, l64 = target.double()[None], lnd.double()[None]
    ch_hist, lnd_hist = [], []
    for it in range(iters):
        z["z"].grad = None
        gen = (O.decode(P, z["z"], topo) * std + mean).double()
        d = _pair_sq(gen, t64.expand(n_starts, -1, -1))
        for name, dd in (("gen->target", d), ("target->gen", d.transpose(1, 2))):
            two = torch.topk(dd.detach(), 2, dim=-1, largest=False).values
            gap = ((two[..., 1] - two[..., 0]) / two[..., 0]).min().item()
            assert gap > 1e-5, f"iteration {it} {name}: best and second-best within {gap:.2e} (pin another seed)"
        ch = (d.min(2).values.mean(1) + d.min(1).values.mean(1)).mean()
        ln = ((gen[:, lidx] - l64) ** 2).mean()
        (10.0 * ln + ch).backward()
        opt.step(z, {"z": z["z"].grad.detach().clone()})
        ch_hist.append(ch.item())
        lnd_hist.append(ln.item())
    print(f"fit mirror: chamfer {ch_hist} / {res.chamfer_history.tolist()}, "
          f"landmark {lnd_hist} / {res.landmark_history.tolist()}")
    np.testing.assert_allclose(res.chamfer_history.cpu().numpy(), ch_hist, rtol=1e-4)
    np.testing.assert_allclose(res.landmark_history.cpu().numpy(), lnd_hist, rtol=1e-4)
    ref_z = z["z"].detach()
    err, tol = (res.z_all.cpu() - ref_z).abs().max().item(), 1e-4 * (1 + ref_z.abs().max().item())
    assert err <= tol, f"z after {iters} steps: max err {err:.3e} > {tol:.3e}"
    assert (ref_z - res.z_init.cpu()).abs().max().item() > 1e-3  # the steps moved z


# ------------------------------------------------------------------ 8. the real size
def test_fit_points_craniofacial_self_consistency(topo_npz):
    spirals, down, up = _ref_inputs(topo_npz)
    net = M.Model(3, recipe.OUT_CH, recipe.LATENT, spirals, down, up, is_vae=True).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    net.eval()
    frozen_names = {"en_layers.0.conv.layer.bias", "de_layers.3.conv.layer.weight"}
    for name, p in net.named_parameters():
        p.requires_grad_(name not in frozen_names)
    flags = {name: p.requires_grad for name, p in net.named_parameters()}
    modes = [m.training for m in net.modules()]
    meshes = recipe.load_meshes()
    mean, std = torch.from_numpy(meshes["norm_mean"]).float(), torch.from_numpy(meshes["norm_std"]).float()
    g = torch.Generator().manual_seed(5)
    z_star = 0.5 * torch.randn(1, recipe.LATENT, generator=g)
    lidx = recipe.sample_idx(17039, k=12, seed=3).tolist()
    with torch.no_grad():
        full = net.decode(z_star.to(DEV))[0] * std.to(DEV) + mean.to(DEV)
    target = full[torch.randperm(17039, generator=g).to(DEV)].contiguous()
    lnd = full[lidx].contiguous()

    def start_losses(zz):
        with torch.no_grad():
            v = net.decode(zz) * std.to(DEV) + mean.to(DEV)
            ch = ops.chamfer_distance(v, target[None], batch_reduction=None)[0]
            ln = ((v[:, lidx] - lnd[None]) ** 2).reshape(zz.shape[0], -1).mean(1)
        return 10.0 * ln + ch

    res = fitting.fit_points(net.decode, target, lnd, lidx, mean, std, torch.zeros(recipe.LATENT), n_starts=16,
                             iterations=20, seed=1)
    assert res.errors_shape.shape == (16,) and res.chamfer_history.shape == (20,)
    first = start_losses(res.z_init)[res.best].item()
    last = (10.0 * res.errors_lnd + res.errors_shape)[res.best].item()
    print(f"craniofacial fit, best start {res.best}: total loss {first:.6g} -> {last:.6g} "
          f"(ratio {last / first:.4f}) after 20 iterations")
    assert last < first
    assert {name: p.requires_grad for name, p in net.named_parameters()} == flags
    assert [m.training for m in net.modules()] == modes
    assert all(p.grad is None for p in net.parameters())
