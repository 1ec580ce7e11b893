"""The rasteriser and shader of csrc/render.hip against a float64 NumPy
restatement of the convention, written out below: one
vectorised pass over the image per face.

pytorch3d, whose conventions these are, is not installed anywhere this suite
runs, so the oracle IS the specification: inclusive edges, no culling, faces
with a vertex at z <= znear dropped, perspective-correct barycentrics, the
nearest depth and on equal bits the lowest face.

Bounds.  eps = 2^-23.  The edge functions are differences of products of O(1)
coordinates, each a few eps off; a barycentric weight divides one by the
face's area A (NDC), so |d bary| <= 64 eps / |A| leaves an order of magnitude;
the depth is 4 x that, relative; a shaded value mixes three O(1) colours with
the weights: 4 x the weight bound + 1e-5.  Pixels where float32 may
legitimately pick another face are excluded as AMBIGUOUS: within 1e-3 pixel
of an edge of a face that (nearly) contains them, or with the two nearest
depths closer than 1e-4 relative; their share is capped at 1 % and the cap is
asserted on the oracle's own mask."""
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
ZNEAR = 1.0


@pytest.fixture(scope="module")
def mods():
    cfsd_loader.load()
    from craniofacialsd_vae_amd import ops, rendering
    return ops, rendering


# ------------------------------------------------------------------ the oracle
def pixel_centres(size):
    c = 1.0 - (2.0 * np.arange(size) + 1.0) / size
    return c[None, :].repeat(size, 0), c[:, None].repeat(size, 1)  # px [i, j] = c[j], py [i, j] = c[i]


def raster64(ndc, vz, faces, size, znear=ZNEAR, crop=False):
    """ndc [V, 2], vz [V] float64, faces [F, 3].  Returns a dict: face [S, S]
    (-1 background), z, bary [S, S, 3], area [S, S] (the winner's triangle
    area), ambiguous [S, S], tie [S, S] (the two nearest depths are equal).
    ``crop``: a face's pass visits only its pixel box grown by two pixels, not
    the image; every pixel the face covers, or comes within the edge tolerance
    of, lies inside it, so the result is the same (test_render_host.py shows
    it)."""
    gx, gy = pixel_centres(size)
    best = np.full((size, size), np.inf)
    second = np.full((size, size), np.inf)
    face = np.full((size, size), -1, np.int64)
    bary = np.full((size, size, 3), -1.0)
    area = np.zeros((size, size))
    edge_amb = np.zeros((size, size), bool)
    tol = 1e-3 * 2.0 / size  # 1e-3 pixel in NDC units
    whole = (slice(None), slice(None))
    for f, (i0, i1, i2) in enumerate(np.asarray(faces)):
        x, y, z = ndc[[i0, i1, i2], 0], ndc[[i0, i1, i2], 1], vz[[i0, i1, i2]]
        if (z <= znear).any():
            continue
        a = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if a == 0.0:
            continue
        box = whole
        if crop:  # pixel j has its centre at 1 - (2j + 1) / S: j = ((1 - c) S - 1) / 2
            j0, j1 = ((1.0 - x.max()) * size - 1.0) / 2, ((1.0 - x.min()) * size - 1.0) / 2
            r0, r1 = ((1.0 - y.max()) * size - 1.0) / 2, ((1.0 - y.min()) * size - 1.0) / 2
            if not all(map(np.isfinite, (j0, j1, r0, r1))):
                raise ValueError("raster64(crop=True) needs finite coordinates")
            if np.ceil(j0 - 0.01) > np.floor(j1 + 0.01) or np.ceil(r0 - 0.01) > np.floor(r1 + 0.01):
                continue  # no pixel centre within 0.01 pixel (ten tolerances) of the face's box
            j0, j1 = max(int(np.floor(j0)) - 2, 0), min(int(np.ceil(j1)) + 2, size - 1)
            r0, r1 = max(int(np.floor(r0)) - 2, 0), min(int(np.ceil(r1)) + 2, size - 1)
            if j0 > j1 or r0 > r1:
                continue
            box = (slice(r0, r1 + 1), slice(j0, j1 + 1))
        px, py = gx[box], gy[box]
        sgn = 1.0 if a > 0 else -1.0
        w, dist = [], []
        for p, q in ((1, 2), (2, 0), (0, 1)):  # w_k: the edge opposite corner k
            wk = (x[q] - x[p]) * (py - y[p]) - (y[q] - y[p]) * (px - x[p])
            w.append(wk)
            ln = np.hypot(x[q] - x[p], y[q] - y[p])
            dist.append(sgn * wk / ln if ln > 0 else np.full_like(wk, np.inf))
        dist = np.stack(dist)
        near = (dist >= -tol).all(0)  # the face grown by the tolerance contains the pixel
        edge_amb[box] |= near & (np.abs(dist) <= tol).any(0)
        inside = (sgn * w[0] >= 0) & (sgn * w[1] >= 0) & (sgn * w[2] >= 0)
        if not inside.any():
            continue
        t = np.stack([w[k] / a / z[k] for k in range(3)], -1)
        with np.errstate(divide="ignore", invalid="ignore"):  # pixels off the face: unused values
            zz = 1.0 / t.sum(-1)
            closer = inside & (zz < best[box])  # strict: equal depth keeps the lower face
            second[box] = np.where(closer, np.minimum(best[box], second[box]),
                                   np.where(inside, np.minimum(second[box], zz), second[box]))
            bary[box] = np.where(closer[..., None], t * zz[..., None], bary[box])
        best[box] = np.where(closer, zz, best[box])
        face[box] = np.where(closer, f, face[box])
        area[box] = np.where(closer, abs(a) / 2, area[box])
    hit = face >= 0
    with np.errstate(invalid="ignore"):
        depth_amb = hit & (second - best < 1e-4 * best)
    return {"face": face, "z": np.where(hit, best, -1.0), "bary": bary, "area": area,
            "ambiguous": edge_amb | depth_amb, "tie": hit & (second == best)}


def normals64(verts, faces):
    n = np.zeros_like(verts)
    for i0, i1, i2 in np.asarray(faces):  # ascending faces
        c = np.cross(verts[i1] - verts[i0], verts[i2] - verts[i0])
        n[i0] += c
        n[i1] += c
        n[i2] += c
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def gouraud64(verts, faces, centre, tex, light=(0.0, 0.0, 3.0), ambient=0.5, diffuse=1.0, specular=0.2,
              shininess=0.5):
    n = normals64(verts, faces)
    l, v = unit(np.asarray(light) - verts), unit(centre - verts)
    nl = (n * l).sum(-1, keepdims=True)
    r = 2 * nl * n - l
    spec = np.where(nl > 0, np.maximum((r * v).sum(-1, keepdims=True), 0.0) ** shininess, 0.0)
    return (ambient + diffuse * np.maximum(nl, 0.0)) * tex + specular * spec


def image64(ras, faces, colors, background=0.0):
    """[3, S, S] from the oracle's raster stage and vertex colours [V, 3]."""
    f = np.where(ras["face"] >= 0, ras["face"], 0)
    img = (ras["bary"][..., None] * colors[np.asarray(faces)[f]]).sum(-2)  # [S, S, 3]
    return np.where((ras["face"] >= 0)[..., None], img, background).transpose(2, 0, 1)


# ------------------------------------------------------------------ scene 1: exact
def exact_scene():
    """Projected vertices on the 1/16 grid (pixel centres of a 16 x 16 image
    are its odd multiples), depths in {1.5, 2, 3}: every edge function is
    exact in float32 and float64 alike, so the owners must agree everywhere."""
    pts, faces = [], []

    def tri(corners, depths):
        base = len(pts)
        for (x, y), z in zip(corners, depths):
            pts.append((x / 16.0, y / 16.0, z))
        faces.append((base, base + 1, base + 2))

    # 0, 1: a square cut along a diagonal THROUGH pixel centres; its corners are pixel centres too
    pts.extend([(15 / 16, 15 / 16, 2.0), (7 / 16, 15 / 16, 2.0), (7 / 16, 7 / 16, 2.0), (15 / 16, 7 / 16, 2.0)])
    faces.extend([(0, 1, 2), (0, 2, 3)])
    tri([(-1, 15), (-9, 15), (-5, 9)], (2.0, 2.0, 2.0))    # 2
    faces.append(faces[2])                                   # 3: its coplanar duplicate (the lower index wins)
    tri([(13, -3), (5, -3), (9, -9)], (1.5, 1.5, 1.5))     # 4: near, listed first
    tri([(15, -1), (1, -1), (8, -15)], (3.0, 3.0, 3.0))    # 5: far, around it
    tri([(-1, -1), (-15, -1), (-8, -15)], (3.0, 3.0, 3.0))  # 6: far, listed first
    tri([(-3, -3), (-11, -3), (-7, -9)], (1.5, 1.5, 1.5))  # 7: near, inside it
    tri([(9, 9), (11, 11), (13, 13)], (1.5, 1.5, 1.5))     # 8: zero area, on the diagonal, nearest: draws nothing
    tri([(40, 40), (-40, 40), (0, -60)], (1.0, 1.5, 1.5))  # 9: covers the image, one vertex at znear: dropped
    tri([(-10, 7), (-30, 7), (-10, 1)], (2.0, 2.0, 2.0))   # 10: partly outside the image
    tri([(20, 20), (30, 20), (25, 30)], (2.0, 2.0, 2.0))   # 11: wholly outside
    tri([(13, 5), (8, 1), (3, 5)], (1.5, 2.0, 3.0))        # 12: the other winding (drawn), sloped
    p = np.asarray(pts, np.float64)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p[:, :2].copy(), p[:, 2].copy(), np.asarray(faces, np.int32)


def test_exact_scene_owners_match_everywhere(mods):
    ops, _ = mods
    ndc, vz, faces = exact_scene()
    ref = raster64(ndc, vz, faces, 16)
    ptf, zbuf, bary = ops.rasterize_ndc(torch.from_numpy(ndc.astype(np.float32))[None].cuda(),
                                        torch.from_numpy(vz.astype(np.float32))[None].cuda(),
                                        torch.from_numpy(faces).cuda(), 16, znear=ZNEAR)
    got = ptf[0].cpu().numpy()
    want = ref["face"]
    # the oracle itself shows what the scene is meant to show
    a0, a1 = faces[0], faces[1]
    assert (ndc[a0[0]] == ndc[a1[0]]).all() and (ndc[a0[2]] == ndc[a1[1]]).all()  # the shared diagonal
    diag = [want[k, k] for k in range(0, 5)]  # pixel centres ON it (15/16 .. 7/16): one owner, the lower face
    assert diag == [0, 0, 0, 0, 0] and want[0, 0] == 0 and want[4, 4] == 0  # ... the corners are vertices
    assert set(np.unique(want)) == {-1, 0, 1, 2, 4, 5, 6, 7, 10, 12}  # 3, 8, 9, 11 own nothing
    assert (want[:, 15] == 10).any() and (want == 5).any() and (want == 6).any()
    square = want[0:5, 0:5]
    upper = np.triu(np.ones((5, 5), bool))
    assert (square[upper] == 0).all() and (square[~upper] == 1).all()  # no hole, one owner each
    assert np.array_equal(got, want), f"owners differ at {np.argwhere(got != want).tolist()}"
    hit = want >= 0
    z, b = zbuf[0].cpu().numpy(), bary[0].cpu().numpy()
    assert (z[~hit] == -1).all() and (b[~hit] == -1).all()
    np.testing.assert_allclose(z[hit], ref["z"][hit], rtol=8 * EPS)
    np.testing.assert_allclose(b[hit], ref["bary"][hit], atol=8 * EPS)


# ------------------------------------------------------------------ scene 2: an icosphere
def icosphere(levels=2):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int32)


SCALES = [(0.9, 1.1, 0.8), (0.7, 0.8, 1.0), (1.0, 0.6, 0.9)]
SHIFT = (0.03, -0.02, 0.01)
SIZES = (64, 48, 20, 44, 100)  # 20, 44, 100: partial tiles on the right and at the bottom
_SCENE = {}


@pytest.fixture(scope="module")
def scene(mods):
    return sphere_scene(mods[1])


def sphere_scene(rendering):
    """The three spheres (float32 vertices; the last vertex belongs to no
    face), their device copies, and per image size the oracle of each mesh:
    raster stage, Gouraud and shadeless images.  Computed once per process
    (test_gpu_render_walk.py uses it too)."""
    if not _SCENE:
        _SCENE.update(_sphere_scene(rendering))
    return _SCENE


def _sphere_scene(rendering):
    v, faces = icosphere(2)
    assert faces.shape == (320, 3)
    v = np.concatenate([v, [[0.0, 0.0, 0.2]]])  # isolated
    verts = np.stack([v * np.asarray(s) + np.asarray(SHIFT) for s in SCALES]).astype(np.float32)
    cam = rendering.look_at()
    rs = np.random.RandomState(5)
    colors = rs.rand(3, len(v), 3).astype(np.float32)
    v64 = verts.astype(np.float64)
    ref = {}
    for size in SIZES:
        per = []
        for k in range(3):
            ndc, vz = cam.project(v64[k])
            ras = raster64(ndc, vz, faces, size)
            ras["gouraud"] = image64(ras, faces, gouraud64(v64[k], faces, cam.centre, 0.5))
            ras["flat"] = image64(ras, faces, colors[k].astype(np.float64), background=0.25)
            per.append(ras)
        ref[size] = per
    return {"verts": verts, "faces": faces, "colors": colors, "cam": cam, "ref": ref,
            "d_verts": torch.from_numpy(verts).cuda(), "d_faces": torch.from_numpy(faces).cuda(),
            "d_colors": torch.from_numpy(colors).cuda()}


def bary_bound(ras, ok):
    return 64 * EPS / ras["area"][ok]


@pytest.mark.parametrize("size", SIZES)
def test_icosphere_raster_stage(mods, scene, size):
    ops, _ = mods
    ptf, zbuf, bary = ops.rasterize_meshes(scene["d_verts"], scene["d_faces"], scene["cam"], size)
    assert ptf.dtype == torch.int32 and tuple(ptf.shape) == (3, size, size) and tuple(bary.shape) == (3, size, size, 3)
    for k in range(3):
        ras = scene["ref"][size][k]
        share = ras["ambiguous"].mean()
        print(f"S={size} mesh {k}: ambiguous share {share:.4%}, covered {np.mean(ras['face'] >= 0):.1%}")
        assert share <= 0.01  # the cap, on the oracle's own mask
        got = ptf[k].cpu().numpy()
        clear = ~ras["ambiguous"]
        assert np.array_equal(got[clear], ras["face"][clear]), \
            f"mesh {k}: {(got[clear] != ras['face'][clear]).sum()} unambiguous pixels have another owner"
        ok = clear & (ras["face"] >= 0)
        assert ok.mean() > 0.2
        bound = bary_bound(ras, ok)
        db = np.abs(bary[k].cpu().numpy()[ok].astype(np.float64) - ras["bary"][ok]).max(-1)
        dz = np.abs(zbuf[k].cpu().numpy()[ok].astype(np.float64) - ras["z"][ok]) / ras["z"][ok]
        print(f"  max |d bary| / bound {np.max(db / bound):.3g}, max |dz|/z / (4 bound) {np.max(dz / (4 * bound)):.3g}")
        assert (db <= bound).all()
        assert (dz <= 4 * bound).all()
        bg = clear & (ras["face"] < 0)
        assert (zbuf[k].cpu().numpy()[bg] == -1).all() and (bary[k].cpu().numpy()[bg] == -1).all()


@pytest.mark.parametrize("size", SIZES)
def test_icosphere_shading(mods, scene, size):
    ops, rendering = mods
    gour = rendering.render(scene["d_verts"], scene["d_faces"], image_size=size).cpu().numpy()
    flat = rendering.render(scene["d_verts"], scene["d_faces"], scene["d_colors"], shading="none", image_size=size,
                            background=0.25).cpu().numpy()
    assert gour.shape == (3, 3, size, size) and gour.dtype == np.float32
    for k in range(3):
        ras = scene["ref"][size][k]
        clear = ~ras["ambiguous"]
        ok = clear & (ras["face"] >= 0)
        tol = 4 * bary_bound(ras, ok) + 1e-5
        for name, got, bgv in (("gouraud", gour[k], 0.0), ("shadeless", flat[k], 0.25)):
            d = np.abs(got[:, ok].astype(np.float64) - ras[name if name == "gouraud" else "flat"][:, ok]).max(0)
            print(f"S={size} mesh {k} {name}: max |d| / tol {np.max(d / tol):.3g}")
            assert (d <= tol).all()
            bg = clear & (ras["face"] < 0)
            assert (got[:, bg] == np.float32(bgv)).all()  # bit-equal background
        assert gour[k].max() > 0.5 and gour[k][:, ok].min() > 0.2  # lit, and the ambient floor 0.5 * 0.5


def test_vertex_normals_and_gouraud_colors(mods, scene):
    ops, rendering = mods
    got = ops.vertex_normals(scene["d_verts"], scene["d_faces"]).cpu().numpy()
    for k in range(3):
        ref = normals64(scene["verts"][k].astype(np.float64), scene["faces"])
        assert np.abs(got[k] - ref).max() <= 1e-6
        assert (got[k, -1] == 0).all()  # the isolated vertex
        np.testing.assert_allclose(np.linalg.norm(got[k, :-1], axis=1), 1.0, atol=1e-6)
    tex = scene["d_colors"]
    col = rendering.gouraud_colors(scene["d_verts"], scene["d_faces"], scene["cam"], tex=tex).cpu().numpy()
    for k in range(3):
        ref = gouraud64(scene["verts"][k].astype(np.float64), scene["faces"], scene["cam"].centre,
                        scene["colors"][k].astype(np.float64))
        # sqrt near zero: an error e of r.V becomes sqrt(e) in spec; e ~ 1e-6 covers the float32 dots
        assert np.abs(col[k, :-1] - ref[:-1]).max() <= 1e-5 + 0.2 * 1e-3


# ------------------------------------------------------------------ determinism
def test_bits_do_not_depend_on_call_batch_or_face_order(mods, scene):
    for size in (64, 44):  # whole tiles only, and partial ones on two sides
        _bits_do_not_depend_on_call_batch_or_face_order(mods, scene, size)


def _bits_do_not_depend_on_call_batch_or_face_order(mods, scene, size):
    ops, rendering = mods
    dv, df, dc = scene["d_verts"], scene["d_faces"], scene["d_colors"]

    def run(verts, faces, colors):
        ndc, vz, _ = ops.project_vertices(verts, scene["cam"])
        return ops.rasterize_ndc(ndc, vz, faces, size, colors=colors, background=0.1)

    first, again = run(dv, df, dc), run(dv, df, dc)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    g0 = rendering.render(dv, df, image_size=size)
    assert torch.equal(g0, rendering.render(dv, df, image_size=size))
    for k in range(3):  # a mesh alone gives the bits it gives in the batch
        alone = run(dv[k:k + 1].contiguous(), df, dc[k:k + 1].contiguous())
        for a, b in zip(first, alone):
            assert torch.equal(a[k:k + 1], b)
        assert torch.equal(g0[k:k + 1], rendering.render(dv[k:k + 1].contiguous(), df, image_size=size))
    again_interp = ops.interpolate_vertex_colors(first[0], first[2], df, dc, background=0.1)
    assert torch.equal(again_interp, first[3])  # the separate operator is the epilogue's arithmetic
    perm = np.random.RandomState(9).permutation(len(scene["faces"]))
    shuffled = run(dv, torch.from_numpy(scene["faces"][perm]).cuda(), dc)
    assert torch.equal(shuffled[1], first[1]) and torch.equal(shuffled[3], first[3])  # zbuf, image
    assert torch.equal(shuffled[2], first[2])
    for k in range(3):
        clear = ~scene["ref"][size][k]["ambiguous"]
        a, b = first[0][k].cpu().numpy(), shuffled[0][k].cpu().numpy()
        assert ((a >= 0) == (b >= 0)).all()
        mapped = np.where(b >= 0, perm[np.maximum(b, 0)], -1)
        assert np.array_equal(mapped[clear], a[clear])


# ------------------------------------------------------------------ real size
def test_two_heads_at_256_are_self_consistent(mods, topo_npz):
    ops, rendering = mods
    verts = torch.from_numpy(recipe.load_meshes()["verts"][:2].astype(np.float32)).cuda()
    faces = torch.from_numpy(np.asarray(topo_npz["face_0"], np.int32)).cuda()
    cam, size = rendering.look_at(), 256
    nv, nf = verts.shape[1], faces.shape[0]
    ndc, vz, _ = ops.project_vertices(verts, cam)
    ptf, zbuf, bary = ops.rasterize_ndc(ndc, vz, faces, size, znear=cam.znear)
    hit = ptf >= 0
    share = hit.double().mean().item()
    print(f"{nf} faces, {nv} vertices: covered share {share:.1%}")
    assert 0.10 <= share <= 0.90
    assert int(ptf.max()) < nf and int(ptf.min()) == -1
    assert bool((zbuf[~hit] == -1).all()) and bool((bary[~hit] == -1).all())
    # the reported face, recomputed in float64 from the projected vertices the kernel was given
    c = 1.0 - (2.0 * torch.arange(size, dtype=torch.float64, device="cuda") + 1.0) / size
    b_i, y_i, x_i = torch.nonzero(hit, as_tuple=True)
    px, py = c[x_i], c[y_i]
    corner = faces[ptf[hit].long()].long()  # [P, 3]
    xy = ndc.double()[b_i[:, None], corner]  # [P, 3, 2]
    z = vz.double()[b_i[:, None], corner]
    x, y = xy[..., 0], xy[..., 1]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    w = torch.stack([(x[:, q] - x[:, p]) * (py - y[:, p]) - (y[:, q] - y[:, p]) * (px - x[:, p])
                     for p, q in ((1, 2), (2, 0), (0, 1))], -1) / area[:, None]
    assert bool((z > cam.znear).all())
    assert w.min().item() >= -1e-4, f"a pixel lies outside its face: {w.min().item()}"
    t = w / z
    zz = 1.0 / t.sum(-1)
    assert ((zz - zbuf[hit].double()).abs() / zz).max().item() <= 1e-4
    assert (t * zz[:, None] - bary[hit].double()).abs().max().item() <= 1e-4
    img = rendering.render(verts, faces)
    assert tuple(img.shape) == (2, 3, 256, 256) and img.dtype == torch.float32
    assert bool(torch.isfinite(img).all())
    assert bool((img.permute(0, 2, 3, 1)[~hit] == 0).all()) and bool((img.permute(0, 2, 3, 1)[hit] > 0).all())


# ------------------------------------------------------------------ the manager
CONFIG = {
    "optimization": {"epochs": 1, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
    "logging_frequency": {"tb_renderings": 1, "save_weights": 100},
}


def test_manager_render_and_log_images(mods, tmp_path, topo_npz):
    ops, rendering = mods
    from craniofacialsd_vae_amd import manager as M
    from craniofacialsd_vae_amd import precompute
    from test_render_host import decode_png
    d = tmp_path
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": 89.11,
                             "swap_features": False, "stratified_split": False})
    cfg["optimization"] = dict(CONFIG["optimization"], latent_consistency_weight=0.0)
    man = M.ModelManager(cfg, device="cuda", precomputed_storage_path=cfg["data"]["precomputed_path"], seed=3,
                         use_graph=False)
    man.engine.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    m = recipe.load_meshes()
    raw = torch.from_numpy(m["verts"][:5].astype(np.float32)).cuda()
    norm = {"mean": torch.from_numpy(m["norm_mean"].astype(np.float32)),
            "std": torch.from_numpy(m["norm_std"].astype(np.float32))}
    shaded = man.render(raw)
    assert tuple(shaded.shape) == (5, 3, 256, 256) and shaded.dtype == torch.float32 and shaded.is_cuda
    errors = torch.linspace(0, 6, raw.shape[1], device="cuda").expand(5, -1).contiguous()
    coloured = man.render(raw, errors, 5)
    assert tuple(coloured.shape) == (5, 3, 256, 256)
    covered = shaded.sum(1) > 0
    assert 0.1 < covered.float().mean().item() < 0.9
    assert bool((coloured.sum(1)[~covered] == 0).all()) and bool((coloured.sum(1)[covered] > 0).all())
    table = torch.from_numpy(rendering.plasma_table().astype(np.float32) / 255).cuda()
    assert coloured.amax().item() <= table.max().item() + 1e-6  # convex mixes of table entries
    x = (raw - norm["mean"].cuda()) / norm["std"].cuda()
    path = man.log_images(x, str(d / "renderings"), 6, norm, phase="validation", error_max_scale=5)
    assert path == str(d / "renderings" / "validation_00000007.png") and os.listdir(d / "renderings") == \
        ["validation_00000007.png"]
    w, h, rgb = decode_png(path)
    assert (w, h) == (4 * (768 + 10) + 10, 2 * (256 + 10) + 10)  # 5 pictures, 4 per row (no swap)
    assert (rgb[:10] == 255).all() and (rgb[:, :10] == 255).all()  # the white frame
    cell = rgb[10:266, 10:778]  # the first mesh: ground truth | reconstruction | errors
    for panel in (cell[:, :256], cell[:, 256:512], cell[:, 512:]):
        assert (panel.reshape(-1, 3).sum(1) > 0).mean() > 0.05  # none is all background
    assert (rgb[276:532, 788:1566] == 255).all()  # an empty cell of the second row
