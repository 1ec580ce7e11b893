"""The point-to-triangle kernels (cfsd_point_face, cfsd_point_face_bwd),
ops.point_face_distance / point_mesh_distance / surface_distance and the
surface path of the latent fitting loop on the GPU.

Oracle: ``tri_closest64`` below, float64, brute force over all faces: the
nearest of the clamped projections onto the three edges and (where it falls
inside) the plane projection -- every candidate is a point of the triangle,
so a zero-area face needs no special case.  tests/test_surface_host.py checks
it against dense barycentric sampling.

Tolerance: |d2 - d2_64| <= C * 2^-24 * L^2, L the distance of the point to
the farthest corner of the oracle's winning face (the error of the difference
form scales with the lengths it subtracts, not with d2: near the surface d2's
relative error is unbounded).  A returned face passes when d64(p, face[idx])
<= min_f d64 + the same bound (tie-robust: no case is excluded).
MEASURED: every check prints the C its inputs need (``worst C so far``); over
this file's seeded inputs the worst on an MI355X was 3.51, at the
craniofacial sample (random faces: 2.71), and WORST_C_MEASURED holds it.  C
is four times that, 14.04, to cover compiler re-association across ROCm
versions; the cap is 256.
Gradients are compared with float64 autograd of the same closest-point
formula THROUGH THE KERNEL'S OWN FACE INDICES: 1e-5 * (1 + max|ref|).  The
fit loop is held to the project's step tolerance, 1e-4 relative.
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
G = ops.PF_GROUP
WORST_C_MEASURED = 3.51
C_TOL = 4 * WORST_C_MEASURED
assert C_TOL <= 256
EPS = 2.0 ** -24
_worst = {"c": 0.0}


# ------------------------------------------------------------------ float64 oracle
def _seg64(p, a, b):
    """Squared distance of p to the segment [a, b] and the parameter t of the nearest point."""
    ab, ap = b - a, p - a
    den = (ab * ab).sum(-1)
    t = torch.where(den > 0, (ap * ab).sum(-1) / den.clamp_min(1e-300), torch.zeros_like(den)).clamp(0, 1)
    e = ap - t[..., None] * ab
    return (e * e).sum(-1), t


def _cross(x, y):
    return torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                        x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def tri_closest64(p, a, b, c):
    """Squared distance of points p [..., 3] to the closed triangles (a, b, c)
    [..., 3] (broadcast; float64) and the barycentric weights [..., 3] of the
    nearest point.  Differentiable."""
    d_ab, t_ab = _seg64(p, a, b)
    d_ac, t_ac = _seg64(p, a, c)
    d_bc, t_bc = _seg64(p, b, c)
    zero, one = torch.zeros_like(d_ab), torch.ones_like(d_ab)
    d2, w = d_ab, torch.stack([one - t_ab, t_ab, zero], -1)
    better = d_ac < d2
    d2, w = torch.where(better, d_ac, d2), torch.where(better[..., None], torch.stack([one - t_ac, zero, t_ac], -1), w)
    better = d_bc < d2
    d2, w = torch.where(better, d_bc, d2), torch.where(better[..., None], torch.stack([zero, one - t_bc, t_bc], -1), w)
    ab, ac, ap = b - a, c - a, p - a
    n = _cross(ab, ac)
    nn = (n * n).sum(-1)
    safe = nn.clamp_min(1e-300)
    bv = (_cross(ap, ac) * n).sum(-1) / safe
    bw = (_cross(ab, ap) * n).sum(-1) / safe
    bu = 1 - bv - bw
    d_in = (ap * n).sum(-1) ** 2 / safe
    inside = (nn > 0) & (bu >= 0) & (bv >= 0) & (bw >= 0) & (d_in < d2)
    return torch.where(inside, d_in, d2), torch.where(inside[..., None], torch.stack([bu, bv, bw], -1), w)


def _corners(verts, faces):
    """a, b, c [Bv, F, 3] of verts [Bv, V, 3], faces [F, 3]."""
    f = faces.long()
    return verts[:, f[:, 0]], verts[:, f[:, 1]], verts[:, f[:, 2]]


def brute64(points, verts, faces, chunk=1 << 21):
    """All-faces float64 search, in chunks of points: (min d2 [B, N], arg min [B, N])."""
    p64, v64 = points.double(), verts.double()
    bsz = max(p64.shape[0], v64.shape[0])
    p64, v64 = p64.expand(bsz, -1, -1), v64.expand(bsz, -1, -1)
    a, b, c = _corners(v64, faces)
    n, nf = p64.shape[1], faces.shape[0]
    step = max(1, chunk // (nf * bsz))
    dmin, amin = [], []
    for s in range(0, n, step):
        d, _ = tri_closest64(p64[:, s:s + step, None, :], a[:, None], b[:, None], c[:, None])
        m = d.min(-1)
        dmin.append(m.values)
        amin.append(m.indices)
    return torch.cat(dmin, 1), torch.cat(amin, 1)


def d64_of_face(points, verts, faces, idx):
    """float64 (d2, weights) of point (b, i) to face idx[b, i]."""
    p64, v64 = points.double(), verts.double()
    bsz = max(p64.shape[0], v64.shape[0])
    p64, v64 = p64.expand(bsz, -1, -1), v64.expand(bsz, -1, -1)
    vid = faces.long()[idx.long()]  # [B, N, 3]
    corner = [torch.gather(v64, 1, vid[:, :, k, None].expand(-1, -1, 3)) for k in range(3)]
    return tri_closest64(p64, *corner), corner


def _check(points, verts, faces, cull=True, what=""):
    """Kernel against the oracle; returns the kernel's results."""
    dist2, idx, bary = ops.point_face_distance(points, verts, faces, cull=cull)
    bsz, n = max(points.shape[0], verts.shape[0]), points.shape[1]
    assert dist2.shape == (bsz, n) and idx.shape == (bsz, n) and bary.shape == (bsz, n, 3)
    assert dist2.dtype == torch.float32 and idx.dtype == torch.int32 and bary.dtype == torch.float32
    assert bool(torch.isfinite(dist2).all()) and bool(torch.isfinite(bary).all())
    assert int(idx.min()) >= 0 and int(idx.max()) < faces.shape[0]
    dmin, amin = brute64(points, verts, faces)
    (_, _), corner = d64_of_face(points, verts, faces, amin)
    p64 = points.double().expand(bsz, -1, -1)
    far2 = torch.stack([((p64 - c) ** 2).sum(-1) for c in corner]).max(0).values  # L^2
    err = (dist2.double() - dmin).abs()
    c_seen = (err / (EPS * far2)).max().item()
    _worst["c"] = max(_worst["c"], c_seen)
    print(f"{what} B={bsz} N={n} F={faces.shape[0]} cull={cull}: C {c_seen:.2f} (worst C so far {_worst['c']:.2f})")
    bound = C_TOL * EPS * far2
    assert bool((err <= bound).all()), f"dist2 error needs C = {c_seen:.1f} > {C_TOL}"
    (got, _), _ = d64_of_face(points, verts, faces, idx)
    assert bool((got <= dmin + bound).all()), "a returned face is not a nearest face"
    # the weights rebuild the nearest point: sum 1, and |p - sum w_k v_k|^2 is the distance
    assert (bary.sum(-1) - 1).abs().max().item() <= 1e-5
    assert float(bary.min()) >= -1e-6
    return dist2, idx, bary


def _rand(shape, seed, scale=80.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _rand_faces(nf, nv, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, nv, (nf, 3), generator=g, dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------ 1. random shapes
@pytest.mark.parametrize("bp,bv", [(1, 1), (3, 3), (3, 1), (1, 3)])
def test_point_face_matches_float64(bp, bv):
    seed = 0
    for n in (1, 63, 65, 257):
        for nf in (1, G - 1, G + 1, 2 * G + 3):
            seed += 1
            nv = nf + 2
            _check(_rand((bp, n, 3), seed), _rand((bv, nv, 3), 100 + seed), _rand_faces(nf, nv, 200 + seed),
                   what="random")


# ------------------------------------------------------------------ 2. the seven regions
TRI = [[0.0, 0, 0], [4, 0, 0], [0, 3, 0]]
REGIONS = [  # in-plane point, nearest point, weights
    ((1.0, 1.0), (1.0, 1.0), (5 / 12, 1 / 4, 1 / 3)),     # interior
    ((2.0, -1.0), (2.0, 0.0), (0.5, 0.5, 0.0)),           # edge ab
    ((-1.0, 1.5), (0.0, 1.5), (0.5, 0.0, 0.5)),           # edge ac
    ((2.6, 2.3), (2.0, 1.5), (0.0, 0.5, 0.5)),            # edge bc
    ((-1.0, -1.0), (0.0, 0.0), (1.0, 0.0, 0.0)),          # vertex a
    ((5.0, -0.5), (4.0, 0.0), (0.0, 1.0, 0.0)),           # vertex b
    ((-0.5, 4.0), (0.0, 3.0), (0.0, 0.0, 1.0)),           # vertex c
]


@pytest.mark.parametrize("z", [0.7, -0.7])
def test_point_face_seven_regions(z):
    pts = torch.tensor([[[x, y, z] for (x, y), _, _ in REGIONS]], device=DEV)
    verts = torch.tensor([TRI], device=DEV)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    dist2, idx, bary = _check(pts, verts, faces, what="regions")
    want_d = torch.tensor([(x - cx) ** 2 + (y - cy) ** 2 + z * z for (x, y), (cx, cy), _ in REGIONS],
                          dtype=torch.float64)
    want_w = torch.tensor([w for _, _, w in REGIONS], dtype=torch.float64)
    assert (dist2[0].double().cpu() - want_d).abs().max().item() <= 1e-5
    assert (bary[0].double().cpu() - want_w).abs().max().item() <= 1e-5
    assert (bary[0].sum(-1) - 1).abs().max().item() <= 1e-6
    assert bool((idx == 0).all())


# ------------------------------------------------------------------ 3. degenerate faces
def test_point_face_degenerate_faces():
    """A collinear face and two coincident-corner faces near the origin, valid
    random faces far away: the points near the origin win a degenerate face and
    get its segment or point distance; nothing is NaN or Inf."""
    far = _rand((1, 20, 3), 1, scale=5.0) + 300.0
    near = torch.tensor([[[0.0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 5, 0], [0, 5, 4]]], device=DEV)
    verts = torch.cat([far, near], 1)  # near = vertices 20..24
    faces = torch.cat([_rand_faces(18, 20, 2),
                       torch.tensor([[20, 21, 22], [23, 23, 23], [23, 23, 24]], dtype=torch.int32, device=DEV),
                       _rand_faces(15, 20, 3)])
    pts = torch.tensor([[[1.0, 0.5, 0.2], [-1, 0.1, 0], [3, 0, 0.3],          # the collinear face: segment a-b
                         [0.2, 5.1, -0.3], [0.1, 5.2, 2.0], [-0.1, 4.9, 5.0]]],  # the point, the segment 23-24
                       device=DEV)
    for cull in (True, False):
        dist2, idx, bary = _check(pts, verts, faces, cull=cull, what="degenerate")
        assert idx[0, :3].tolist() == [18, 18, 18]
        assert set(idx[0, 3:].tolist()) <= {19, 20}
        p64, v64 = pts[0].double(), verts[0].double()
        seg_ab = _seg64(p64[:3], v64[20], v64[21])[0]
        seg_pt = _seg64(p64[3:], v64[23], v64[24])[0]
        want = torch.cat([seg_ab, seg_pt])
        assert (dist2[0].double() - want).abs().max().item() <= C_TOL * EPS * 30.0


# ------------------------------------------------------------------ 4. ties
def test_point_face_ties_resolve_to_first_copy():
    """Every face three times, the copies in different groups: each point gets
    the FIRST copy, with the bits of the search over the base faces."""
    nf0, nv = 20, 22
    base = _rand_faces(nf0, nv, 5)
    faces = torch.cat([base, base, base])
    verts, pts = _rand((3, nv, 3), 6), _rand((3, 130, 3), 7)
    for cull in (True, False):
        dist2, idx, bary = _check(pts, verts, faces, cull=cull, what="ties")
        assert int(idx.max()) < nf0
        d0, i0, w0 = ops.point_face_distance(pts, verts, base, cull=cull)
        assert torch.equal(idx, i0) and torch.equal(dist2, d0) and torch.equal(bary, w0)


def _torus(nu=24, nv=12):
    pos, faces = ST.torus_grid(nu, nv)
    return (torch.from_numpy(pos.astype(np.float32))[None].to(DEV),
            torch.from_numpy(faces.astype(np.int32)).to(DEV))


def test_point_face_points_nearest_to_a_shared_edge():
    """On the closed torus, points displaced from edge midpoints along the
    radial direction: two faces share the nearest edge."""
    verts, faces = _torus()
    f = faces.long()
    mid = 0.5 * (verts[0, f[:, 0]] + verts[0, f[:, 1]])  # an edge of every face; each is shared by two
    centre = torch.tensor([0.0, 0.0, 0.0], device=DEV)
    pts = (mid + 0.01 * (mid - centre))[None].contiguous()
    d_c, i_c, _ = _check(pts, verts, faces, cull=True, what="shared edge")
    d_b, i_b, _ = _check(pts, verts, faces, cull=False, what="shared edge")
    assert torch.equal(d_c, d_b) and torch.equal(i_c, i_b)


# ------------------------------------------------------------------ 5. group boundaries
@pytest.mark.parametrize("k", [1, 3])
def test_point_face_nearest_face_last_in_partial_group(k):
    nf = G * k + 1
    verts = torch.cat([_rand((2, 30, 3), 8, scale=2.0) + 50.0,
                       torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]], device=DEV).expand(2, -1, -1)], 1)
    faces = torch.cat([_rand_faces(nf - 1, 30, 9), torch.tensor([[30, 31, 32]], dtype=torch.int32, device=DEV)])
    pts = _rand((2, 70, 3), 10, scale=0.3)
    for cull in (True, False):
        _, idx, _ = _check(pts, verts.contiguous(), faces, cull=cull, what="last face")
        assert bool((idx == nf - 1).all())


# ------------------------------------------------------------------ 6. culling is exact
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("nu,nv,bp,bv", [(24, 12, 1, 1), (24, 12, 3, 1), (12, 6, 1, 3), (48, 24, 2, 2)])
def test_culling_is_exact_on_tori(nu, nv, bp, bv):
    _, faces = _torus(nu, nv)
    meshes = torch.from_numpy(ST.torus_meshes(bp + bv, nu=nu, nv=nv, seed=3)).to(DEV)
    pts, verts = meshes[:bp].contiguous(), meshes[bp:].contiguous()
    on = ops.point_face_distance(pts, verts, faces, cull=True, return_stats=True)
    off = ops.point_face_distance(pts, verts, faces, cull=False, return_stats=True)
    assert _same(on[:3], off[:3])
    _check(pts, verts, faces, what="torus")
    waves = on[3].shape[0]
    assert int(off[3][:, 1].sum()) == waves * faces.shape[0]  # brute force evaluates every face
    print(f"torus {nu}x{nv}: culled search evaluates {int(on[3][:, 1].sum()) / (waves * faces.shape[0]):.3f} "
          f"of the faces, enters {int(on[3][:, 0].sum()) / (waves * ((faces.shape[0] + G - 1) // G)):.3f} "
          "of the groups")
    if nu >= 24:
        assert int(on[3][:, 1].sum()) < int(off[3][:, 1].sum())


@pytest.fixture(scope="module")
def cranio(topo_npz):
    m = recipe.load_meshes()["verts"]
    faces = torch.from_numpy(np.asarray(topo_npz["face_0"], np.int32).reshape(-1, 3)).to(DEV)
    return (torch.from_numpy(m[0].astype(np.float32))[None].to(DEV),
            torch.from_numpy(m[5].astype(np.float32))[None].to(DEV), faces)


def test_culling_is_exact_at_craniofacial_size(cranio):
    pts, verts, faces = cranio
    on = ops.point_face_distance(pts, verts, faces, cull=True, return_stats=True)
    off = ops.point_face_distance(pts, verts, faces, cull=False)
    assert _same(on[:3], off)
    waves, nf = on[3].shape[0], faces.shape[0]
    print(f"craniofacial: culled search evaluates {int(on[3][:, 1].sum()) / (waves * nf):.4f} of the faces, "
          f"enters {int(on[3][:, 0].sum()) / (waves * ((nf + G - 1) // G)):.4f} of the groups")
    sel = torch.from_numpy(recipe.sample_idx(pts.shape[1], k=256, seed=11)).to(DEV)
    sub = pts[:, sel].contiguous()
    got = _check(sub, verts, faces, what="craniofacial sample")
    assert torch.equal(got[0], on[0][:, sel]) and torch.equal(got[1], on[1][:, sel])
    # a SurfaceMesh keeps the records: the second search skips the pre-launch, same bits
    mesh = ops.SurfaceMesh(verts, faces)
    first = ops.point_face_distance(pts, mesh)
    assert mesh.prepared
    assert _same(first, off) and _same(ops.point_face_distance(pts, mesh), off)


# ------------------------------------------------------------------ 7. unreferenced vertices
def test_unreferenced_vertices_do_not_seed():
    """Vertices no face uses, exactly AT the query points: they are not on the
    surface; as seeds they would bound every search by zero."""
    verts, faces = _torus()
    pts = (verts * 1.3 + 0.05).contiguous()[:, :100].contiguous()
    ref = ops.point_face_distance(pts, verts, faces)
    more = torch.cat([verts, pts], 1).contiguous()
    got = ops.point_face_distance(pts, more, faces)
    assert float(ref[0].min()) > 1e-4
    assert _same(ref, got)
    _check(pts, more, faces, what="unreferenced")


def test_face_indices_are_checked_once_per_face_tensor():
    verts, faces = _torus(12, 6)
    pts = (verts * 1.2).contiguous()
    for bad in (72, -1):
        f = faces.clone()
        f[5, 1] = bad
        for fn in (ops.point_face_distance, ops.point_mesh_distance):
            with pytest.raises(ValueError):
                fn(pts, verts, f)
        with pytest.raises(ValueError):
            ops.surface_distance(pts, faces, verts, f)
        with pytest.raises(ValueError):
            ops.surface_distance(pts, f, verts, faces)
    with pytest.raises(ValueError):
        ops.point_face_distance(pts, verts, faces.long())
    with pytest.raises(ValueError):
        ops.point_face_distance(pts, verts, faces.reshape(-1))
    with pytest.raises(ValueError):
        ops.point_face_distance(pts[0], verts, faces)
    tab = ops.face_table(faces, 72)
    assert ops.face_table(faces, 72) is tab  # validated once: the table is kept with the tensor
    ops.point_face_distance(pts, verts, faces)
    assert ops.face_table(faces, 72) is tab
    faces[0, 0] = 99  # an in-place change is a new version: validated again
    with pytest.raises(ValueError):
        ops.point_face_distance(pts, verts, faces)


# ------------------------------------------------------------------ 8. gradients
def _grad_ref(points, verts, faces, idx, upstream):
    p64 = points.double().requires_grad_(True)
    v64 = verts.double().requires_grad_(True)
    bsz = max(points.shape[0], verts.shape[0])
    pe, ve = p64.expand(bsz, -1, -1), v64.expand(bsz, -1, -1)
    vid = faces.long()[idx.long()]
    corner = [torch.gather(ve, 1, vid[:, :, k, None].expand(-1, -1, 3)) for k in range(3)]
    d2, _ = tri_closest64(pe, *corner)
    (d2 * upstream.double()).sum().backward()
    return d2.detach(), p64.grad, v64.grad


@pytest.mark.parametrize("bp,bv", [(1, 1), (3, 3), (3, 1), (1, 3)])
def test_point_mesh_distance_gradients(bp, bv):
    verts, faces = _torus(12, 6)
    meshes = torch.from_numpy(ST.torus_meshes(bp + bv, nu=12, nv=6, seed=9)).to(DEV)
    lonely = torch.full((bv, 1, 3), 40.0, device=DEV)  # referenced by one far face nobody wins: an empty run
    faces = torch.cat([faces, torch.tensor([[72, 72, 72]], dtype=torch.int32, device=DEV)])
    outs = []
    for _ in range(2):
        pts = (meshes[:bp] * 1.1 + 0.02).contiguous().requires_grad_(True)
        vs = torch.cat([meshes[bp:], lonely], 1).contiguous().requires_grad_(True)
        d2, idx, bary = ops.point_mesh_distance(pts, vs, faces, return_faces=True)
        upstream = _rand(d2.shape, 12, scale=1.0)
        (d2 * upstream).sum().backward()
        outs.append((d2.detach().clone(), idx.clone(), pts.grad.clone(), vs.grad.clone()))
    assert _same(outs[0], outs[1])  # bitwise deterministic
    d2, idx, gp, gv = outs[0]
    assert gp.shape == pts.shape and gv.shape == vs.shape
    ref_d, ref_gp, ref_gv = _grad_ref(pts.detach(), vs.detach(), faces, idx, upstream)
    assert (d2.double() - ref_d).abs().max().item() <= 1e-5 * (1 + ref_d.abs().max().item())
    for name, got, ref in (("points", gp, ref_gp), ("verts", gv, ref_gv)):
        err, tol = (got.double() - ref).abs().max().item(), 1e-5 * (1 + ref.abs().max().item())
        assert err <= tol, f"grad {name}: {err:.3e} > {tol:.3e}"
    assert ref_gv.abs().max().item() > 1e-3
    assert 72 not in faces.long()[idx.long()].reshape(-1).tolist()
    assert bool((gv[:, 72] == 0).all())


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
    """The 288-vertex torus (levels 288 / 144 / 72 / 36), AE, golden weights;
    its normalisation; z*, decode(z*) and that head midpoint-subdivided."""
    npz = ST.torus_topology(nu=NU, nv=NV, factors=(2, 2, 2))
    shapes = recipe.param_shapes(num_vert=36, out_ch=SMALL_CH, latent=SMALL_LATENT, is_vae=False)
    w = recipe.golden_weights(shapes, seed=4)
    spirals, down, up = _ref_inputs(npz)
    net = M.Model(3, SMALL_CH, SMALL_LATENT, spirals, down, up, is_vae=False).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    pos, faces = ST.torus_grid(NU, NV)
    mean = torch.from_numpy(pos.astype(np.float32))
    std = torch.from_numpy((0.05 + 0.02 * np.cos(np.arange(pos.size)).reshape(pos.shape)).astype(np.float32))
    z_star = torch.randn(1, SMALL_LATENT, generator=torch.Generator().manual_seed(77))
    with torch.no_grad():
        head = net.decode(z_star.to(DEV))[0] * std.to(DEV) + mean.to(DEV)
    sub_v, sub_f = _subdivide(head, faces)
    return dict(net=net, w=w, topo=O.Topology(npz), mean=mean, std=std, z_star=z_star, head=head,
                faces=torch.from_numpy(faces.astype(np.int32)).to(DEV), sub_v=sub_v, sub_f=sub_f)


def _subdivide(verts, faces):
    """Midpoint subdivision: every face becomes four, the same piecewise-linear surface."""
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    uniq, inv = np.unique(edges, axis=0, return_inverse=True)
    nv, nf = verts.shape[0], len(faces)
    m = inv.reshape(-1)
    mab, mbc, mca = nv + m[:nf], nv + m[nf:2 * nf], nv + m[2 * nf:]
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    sub = np.concatenate([np.stack([a, mab, mca], 1), np.stack([mab, b, mbc], 1), np.stack([mca, mbc, c], 1),
                          np.stack([mab, mbc, mca], 1)])
    e = torch.from_numpy(uniq).to(verts.device)
    mids = 0.5 * (verts[e[:, 0]] + verts[e[:, 1]])
    return torch.cat([verts, mids]).contiguous(), torch.from_numpy(sub.astype(np.int32)).to(verts.device)


# ------------------------------------------------------------------ 9. the surface term has no sampling floor
def test_surface_distance_on_subdivided_target(small):
    gen = small["head"][None].contiguous()
    scan, scan_f = small["sub_v"][None].contiguous(), small["sub_f"]
    assert scan.shape[1] == 4 * 288 and scan_f.shape[0] == 4 * small["faces"].shape[0]
    for pts, verts, faces in ((gen, scan, scan_f), (scan, gen, small["faces"])):
        d2, idx, _ = ops.point_face_distance(pts, verts, faces)
        (_, _), corner = d64_of_face(pts, verts, faces, idx)
        far2 = torch.stack([((pts.double() - c) ** 2).sum(-1) for c in corner]).max(0).values
        # (the scan's midpoints are rounded to fp32: truly off their edge by up to 2^-24 per coordinate, |x| < 2)
        assert bool((d2.double() <= C_TOL * EPS * far2 + 3 * EPS ** 2).all())
    surf = ops.surface_distance(gen, small["faces"], scan, scan_f).item()
    cham = ops.chamfer_distance(gen, scan)[0].item()
    print(f"subdivided target at z*: surface term {surf:.3e}, vertex Chamfer {cham:.3e}")
    assert cham >= 1e4 * surf and cham > 1e-4
    per = ops.surface_distance(gen.expand(3, -1, -1).contiguous(), small["faces"], ops.SurfaceMesh(scan, scan_f),
                               batch_reduction=None)
    assert per.shape == (3,) and abs(per.sum().item() / 3 - surf) <= 1e-6 * surf + 1e-20


# ------------------------------------------------------------------ 10. fit loop vs host mirror
def test_fit_points_with_faces_matches_host_mirror(small):
    net, w, topo, mean, std = small["net"], small["w"], small["topo"], small["mean"], small["std"]
    n_starts, iters, lr = 4, 3, 5e-3
    lidx = [3, 61, 118, 176, 233]
    target, tf, gf = small["sub_v"], small["sub_f"], small["faces"]
    lnd = small["head"][lidx].cpu().contiguous()
    res = fitting.fit_points(net.decode, target, lnd, lidx, mean, std, torch.zeros(SMALL_LATENT), n_starts=n_starts,
                             lr=lr, iterations=iters, seed=0, target_faces=tf, template_faces=gf)
    assert res.z_all.shape == (n_starts, SMALL_LATENT) and res.verts.shape == (288, 3)
    assert res.surface_mm is not None and res.errors_shape.shape == (n_starts,)

    # host mirror: oracle decoder (fp32), float64 surface term through the kernel's faces, plain Adam
    P = {k: v.detach() for k, v in O.make_params(w).items()}
    z = {"z": res.z_init.cpu().clone().requires_grad_(True)}
    opt = O.Adam(z, lr=lr)
    t32 = target[None].contiguous()
    t64, l64 = t32.double().cpu(), lnd.double()[None]
    sh_hist, lnd_hist = [], []

    def through_kernel_faces(p64, v64, faces):
        _, idx, _ = ops.point_face_distance(p64.detach().float().to(DEV).contiguous(),
                                            v64.detach().float().to(DEV).contiguous(), faces)
        bsz = max(p64.shape[0], v64.shape[0])
        pe, ve = p64.expand(bsz, -1, -1), v64.expand(bsz, -1, -1)
        vid = faces.long().cpu()[idx.long().cpu()]
        corner = [torch.gather(ve, 1, vid[:, :, k, None].expand(-1, -1, 3)) for k in range(3)]
        return tri_closest64(pe, *corner)[0]

    for it in range(iters):
        z["z"].grad = None
        gen = (O.decode(P, z["z"], topo) * std + mean).double()
        sh = (through_kernel_faces(gen, t64, tf).mean(1) + through_kernel_faces(t64, gen, gf).mean(1)).mean()
        ln = ((gen[:, lidx] - l64) ** 2).mean()
        (10.0 * ln + sh).backward()
        opt.step(z, {"z": z["z"].grad.detach().clone()})
        sh_hist.append(sh.item())
        lnd_hist.append(ln.item())
    print(f"surface fit mirror: surface {sh_hist} / {res.chamfer_history.tolist()}, "
          f"landmark {lnd_hist} / {res.landmark_history.tolist()}")
    np.testing.assert_allclose(res.chamfer_history.cpu().numpy(), sh_hist, rtol=1e-4)
    np.testing.assert_allclose(res.landmark_history.cpu().numpy(), lnd_hist, rtol=1e-4)
    ref_z = z["z"].detach()
    err, tol = (res.z_all.cpu() - ref_z).abs().max().item(), 1e-4 * (1 + ref_z.abs().max().item())
    assert err <= tol, f"z after {iters} steps: max err {err:.3e} > {tol:.3e}"
    assert (ref_z - res.z_init.cpu()).abs().max().item() > 1e-3  # the steps moved z


# ------------------------------------------------------------------ 11. the real size
def test_fit_points_surface_craniofacial_self_consistency(topo_npz):
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
    gf = torch.from_numpy(np.asarray(topo_npz["face_0"], np.int32).reshape(-1, 3)).to(DEV)
    with torch.no_grad():
        full = net.decode(z_star.to(DEV))[0] * std.to(DEV) + mean.to(DEV)
    perm = torch.randperm(17039, generator=g).to(DEV)  # scan vertex j = head vertex perm[j]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(17039, device=DEV)
    target, tf = full[perm].contiguous(), inv[gf.long()].to(torch.int32).contiguous()
    lnd = full[lidx].contiguous()
    scan = ops.SurfaceMesh(target, tf)

    def start_losses(zz):
        with torch.no_grad():
            v = net.decode(zz) * std.to(DEV) + mean.to(DEV)
            sh = ops.surface_distance(v, gf, scan, batch_reduction=None)
            ln = ((v[:, lidx] - lnd[None]) ** 2).reshape(zz.shape[0], -1).mean(1)
        return 10.0 * ln + sh

    res = fitting.fit_points(net.decode, target, lnd, lidx, mean, std, torch.zeros(recipe.LATENT), n_starts=16,
                             iterations=20, seed=1, target_faces=tf, template_faces=gf)
    assert res.errors_shape.shape == (16,) and res.chamfer_history.shape == (20,)
    first = start_losses(res.z_init)[res.best].item()
    last = (10.0 * res.errors_lnd + res.errors_shape)[res.best].item()
    surface = float(res.surface_mm)
    print(f"craniofacial surface fit, best start {res.best}: total loss {first:.6g} -> {last:.6g} "
          f"(ratio {last / first:.4f}) after 20 iterations; surface distance {surface:.6g}")
    assert last < first
    assert np.isfinite(surface) and surface > 0
    assert {name: p.requires_grad for name, p in net.named_parameters()} == flags
    assert [m.training for m in net.modules()] == modes
    assert all(p.grad is None for p in net.parameters())
