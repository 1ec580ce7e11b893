"""The control flow of rn_raster_k (csrc/render.hip) that the scenes of
test_gpu_render.py never enter, against the same float64 oracle: a second
round of the group walk, several passes of the four-groups-at-a-time loop and
a short last one, ties decided between waves in both directions, partial
tiles and image sides below 8, broadcast colours, vertices that cannot be
projected, and a vertex normal of valence 200.

The lattice scene is exact: all coordinates are dyadic, so every edge
function, weight and depth is the same number in float32 and float64, and the
owners must agree at EVERY pixel; no ambiguity mask is used on it.
test_render_host.py proves that without a GPU, from a float32 NumPy
restatement of the kernel's arithmetic (``raster_np`` below).

A permuted face list must give the same picture.  On the lattice every
covered pixel centre lies on a shared edge or a shared vertex (that is what
makes it a test of ties), so a permutation hands most pixels to ANOTHER of
the tied faces: depth and colour keep their bits, but the barycentric triple
is that face's (the same weights at other corners).  The permuted call is
therefore compared with the oracle of the permuted list, owner by owner, and
its ``bary`` must be bit-equal to the unpermuted call's wherever the owner
maps back to the same face, which includes every pixel that is not a tie."""
import numpy as np
import pytest
import torch

import cfsd_loader
import recipe
from test_gpu_render import EPS, ZNEAR, bary_bound, image64, normals64, raster64, sphere_scene

pytestmark = pytest.mark.gpu
GROUP, WAVES, ROUND = 16, 8, 512  # faces per group box, waves per tile, groups per round of the walk (64 x 8)


@pytest.fixture(scope="module")
def mods():
    cfsd_loader.load()
    from craniofacialsd_vae_amd import ops, rendering
    assert ops.RN_GROUP == GROUP
    return ops, rendering


@pytest.fixture(scope="module")
def scene(mods):
    return sphere_scene(mods[1])


# ------------------------------------------------------------------ the kernel's arithmetic, restated
def raster_np(ndc, vz, faces, size, dtype, znear=ZNEAR, chunk=128, rank=None):
    """The documented arithmetic of rn_setup_k / rn_raster_k in NumPy at
    ``dtype``: difference-form edge functions, t_k = w_k (1 / area) (1 /
    z_k), z = 1 / sum t, the nearest z and on equal bits the lowest face.
    Every operation is one rounding, in the kernel's order (contraction is off
    there).  The kernel's boxes are conservative and left out; a chunk of
    faces is evaluated on the pixel rows and columns its vertices span, grown
    by a pixel.  ``rank`` [F]: what decides between equal depths in the
    face's place (the faces' positions in a permuted list).  Returns face, z,
    bary."""
    ft = np.dtype(dtype).type
    ndc, vz, faces = np.asarray(ndc, dtype), np.asarray(vz, dtype), np.asarray(faces)
    rank = np.arange(len(faces)) if rank is None else np.asarray(rank)
    c = ft(1) - (2 * np.arange(size) + 1).astype(dtype) / ft(size)
    best = np.full((size, size), np.inf, dtype)
    face = np.full((size, size), -1, np.int64)
    prio = np.full((size, size), -1, np.int64)
    bary = np.full((size, size, 3), -1, dtype)
    with np.errstate(all="ignore"):
        for f0 in range(0, len(faces), chunk):
            fc = faces[f0:f0 + chunk]
            x, y, z = ndc[fc, 0], ndc[fc, 1], vz[fc]  # [C, 3]
            box = []
            for v in (y, x):  # rows, columns: pixel u = ((1 - c) S - 1) / 2
                lo, hi = ((1.0 - float(v.max())) * size - 1) / 2, ((1.0 - float(v.min())) * size - 1) / 2
                whole = not (np.isfinite(lo) and np.isfinite(hi))
                box.append(slice(0, size) if whole else
                           slice(int(min(max(np.floor(lo) - 1, 0), size)), int(min(max(np.ceil(hi) + 2, 0), size))))
            py, px = c[box[0]][None, :, None], c[box[1]][None, None, :]
            if py.size == 0 or px.size == 0:
                continue
            x0, x1, x2 = (x[:, k, None, None] for k in range(3))
            y0, y1, y2 = (y[:, k, None, None] for k in range(3))
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            keep = (z > ft(znear)).all(1)[:, None, None] & (np.abs(area) > 0) & (np.abs(area) < np.inf)
            ia, iz = ft(1) / area, (ft(1) / z)[:, :, None, None]
            w0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
            w1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
            w2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
            inside = keep & np.where(ia > 0, (w0 >= 0) & (w1 >= 0) & (w2 >= 0), (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            t = [w0 * ia * iz[:, 0], w1 * ia * iz[:, 1], w2 * ia * iz[:, 2]]
            zz = np.where(inside, ft(1) / (t[0] + t[1] + t[2]), np.inf).astype(dtype)
            rk = rank[f0:f0 + chunk][:, None, None]
            pick = np.where(zz == zz.min(0), rk, np.iinfo(np.int64).max).argmin(0)[None]  # equal depths: the lowest rank
            zc, rc = np.take_along_axis(zz, pick, 0)[0], rk[pick[0], 0, 0]
            closer = (zc < best[box[0], box[1]]) | ((zc == best[box[0], box[1]]) & (zc < np.inf) &
                                                   (rc < prio[box[0], box[1]]))
            sub = (box[0], box[1])
            best[sub] = np.where(closer, zc, best[sub])
            face[sub] = np.where(closer, f0 + pick[0], face[sub])
            prio[sub] = np.where(closer, rc, prio[sub])
            for k in range(3):
                bary[sub + (k,)] = np.where(closer, np.take_along_axis(t[k], pick, 0)[0] * zc, bary[sub + (k,)])
    return {"face": face, "z": np.where(face >= 0, best, ft(-1)), "bary": bary}


def pixel_range(cmin, cmax, size):
    """rn_pixel_range of render.hip in float32: the pixels whose centres may lie in [cmin, cmax]."""
    f = np.float32
    fs, slack = f(size), f(0.015625)
    ulo = ((f(1) - f(cmax)) * fs - f(1)) * f(0.5) - slack
    uhi = ((f(1) - f(cmin)) * fs - f(1)) * f(0.5) + slack
    return int(np.ceil(min(max(ulo, f(0)), fs))), int(np.floor(min(max(uhi, f(-1)), fs - f(1))))


def group_boxes(ndc, vz, faces, size, znear=ZNEAR):
    """Per group of 16 faces the pixel box (x0, x1, y0, y1) that rn_setup_k gives it, or None when empty."""
    out = []
    for g0 in range(0, len(faces), GROUP):
        box = None
        for i0, i1, i2 in faces[g0:g0 + GROUP]:
            x, y, z = ndc[[i0, i1, i2], 0], ndc[[i0, i1, i2], 1], vz[[i0, i1, i2]]
            area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            if (z <= znear).any() or area == 0:
                continue
            xa, xb = pixel_range(x.min(), x.max(), size)
            ya, yb = pixel_range(y.min(), y.max(), size)
            if xa > xb or ya > yb:
                continue
            box = (xa, xb, ya, yb) if box is None else (min(box[0], xa), max(box[1], xb), min(box[2], ya),
                                                         max(box[3], yb))
        out.append(box)
    return out


def entered_groups(boxes, size):
    """[tiles, tiles, WAVES, rounds]: how many group boxes of wave w and round r overlap each 8 x 8 tile."""
    tiles, rounds = -(-size // 8), -(-len(boxes) // ROUND)
    n = np.zeros((tiles, tiles, WAVES, rounds), np.int64)
    for g, box in enumerate(boxes):
        if box is None:
            continue
        for ty in range(tiles):
            for tx in range(tiles):
                qx1, qy1 = min(tx * 8 + 8, size) - 1, min(ty * 8 + 8, size) - 1
                if box[0] <= qx1 and box[1] >= tx * 8 and box[2] <= qy1 and box[3] >= ty * 8:
                    n[ty, tx, g % WAVES, g // ROUND] += 1
    return n


# ------------------------------------------------------------------ scene 3: the lattice
LATTICE_SIZES = (1, 2, 4, 16, 64)  # powers of two: dyadic pixel centres
FAR, NEAR, FILLER, COPIES = 0, 4608, 9216, 9264  # the first face of each part


def sheet(n, x0, y0, h, z, base):
    """(n + 1)^2 vertices (x0 + j h, y0 + i h, z), row-major, and the 2 n^2
    faces of its quads in row-major order: the quad a, b = a + 1, c = a + n +
    1, d = a + n + 2 gives (a, b, d) and (a, d, c)."""
    i, j = np.divmod(np.arange((n + 1) ** 2), n + 1)
    pts = np.stack([x0 + j * h, y0 + i * h, np.full(len(i), z)], -1)
    a = (base + np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    b, c, d = a + 1, a + n + 1, a + n + 2
    return pts, np.stack([np.stack([a, b, d], -1), np.stack([a, d, c], -1)], 1).reshape(-1, 3)


def lattice_scene():
    """Two flat sheets of 48 x 48 quads with the pitch 1/32, the near one
    (z = 2) shifted by (17/64, 9/64) over the far one (z = 4), 48 zero-area
    faces nearer than both, and copies of the far sheet's first 256 faces at
    the end: 9520 faces, 595 groups, two rounds of the walk.  Near faces from
    8192 on are met in round 1 and must beat far winners of round 0; the copy
    of group k is group 579 + k, so it sits in wave (k + 3) mod 8 and the
    original in wave k mod 8: the tie between them is decided in the LDS
    merge, in either direction.  Mesh 1 has the sheets' depths swapped.
    Returns ndc [V, 2], vz [2, V] (float64, exact in float32), faces [F, 3]."""
    far, f_far = sheet(48, -0.75, -0.75, 1 / 32, 4.0, 0)
    near, f_near = sheet(48, -0.75 + 17 / 64, -0.75 + 9 / 64, 1 / 32, 2.0, len(far))
    base = len(far) + len(near)
    fill = np.array([[0.0, 0.0, 1.5], [0.25, 0.25, 1.5], [0.5, 0.5, 1.5]])
    f_fill = np.tile([[base, base + 1, base + 2]], (48, 1))
    pts = np.concatenate([far, near, fill])
    faces = np.concatenate([f_far, f_near, f_fill, f_far[:256]]).astype(np.int32)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    assert pts.shape == (4805, 3) and faces.shape == (9520, 3) and -(-len(faces) // GROUP) == 595
    assert (len(f_far), len(f_far) + len(f_near), len(faces) - 256) == (NEAR, FILLER, COPIES)
    assert COPIES == 579 * GROUP
    swapped = np.where(pts[:, 2] == 4.0, 2.0, np.where(pts[:, 2] == 2.0, 4.0, pts[:, 2]))
    return pts[:, :2].copy(), np.stack([pts[:, 2], swapped]), faces


_LATTICE = {}


def lattice_refs():
    """The scene and raster64 of both meshes at every size, once per process."""
    if not _LATTICE:
        ndc, vz, faces = lattice_scene()
        _LATTICE.update(ndc=ndc, vz=vz, faces=faces,
                        ref={s: [raster64(ndc, vz[m], faces, s, crop=True) for m in range(2)] for s in LATTICE_SIZES})
    return _LATTICE


def check_lattice_facts(lat):
    """What the scene is built to show, asserted on the oracle alone."""
    ndc, vz, faces, ref = lat["ndc"], lat["vz"], lat["faces"], lat["ref"]
    want = {64: (0.707, 511, 128), 16: (0.695, 32, 12)}
    for size, (share, late, low) in want.items():
        own = ref[size][0]["face"]
        assert abs(np.mean(own >= 0) - share) < 5e-4
        assert np.sum(own >= 8192) == late  # met in round 1, in front of round 0's winners
        assert np.sum((own >= 0) & (own < 256)) == low  # originals of the copies
        assert np.sum(own >= COPIES) == 0 and not ((own >= FILLER) & (own < COPIES)).any()
    own0, own1 = ref[64][0]["face"], ref[64][1]["face"]
    assert abs(np.mean(own0 != own1) - 0.43) < 5e-3
    # the copy of group k is group 579 + k: originals in wave k % 8, copies in wave (k + 3) % 8
    groups = np.unique(own0[(own0 >= 0) & (own0 < 256)] // GROUP)
    assert groups.tolist() == list(range(16))
    for k in groups:
        assert np.array_equal(faces[COPIES + k * GROUP:COPIES + (k + 1) * GROUP], faces[k * GROUP:(k + 1) * GROUP])
        assert (COPIES // GROUP + k) % WAVES == (k + 3) % WAVES and (COPIES // GROUP + k) // ROUND == 1
    above = [k for k in groups if k % WAVES > (k + 3) % WAVES]  # the lower face is held by the higher wave
    assert above == [5, 6, 7, 13, 14, 15] and len(groups) - len(above) == 10  # ... and by the lower wave
    assert ref[64][0]["tie"][(own0 >= 0) & (own0 < 256)].all()  # each such pixel IS a tie (with the copy)
    # 16 x 16: some wave of every tile enters more than four groups in one round, and not a multiple of four
    n = entered_groups(group_boxes(ndc, vz[0], faces, 16), 16)
    assert n.shape == (2, 2, WAVES, 2)
    assert (n.max((-1, -2)) >= 16).all()  # four passes of some wave in one round, in every tile
    assert ((n > 4) & (n % 4 != 0)).any((-1, -2)).all()  # a second pass AND a short last pass in one walk
    assert ((n > 0) & (n < 4)).any((-1, -2)).all()  # a walk of one short pass
    for size in (1, 2, 4):  # one partial tile, no background
        for m in range(2):
            assert (ref[size][m]["face"] >= 0).all()


@pytest.fixture(scope="module")
def lattice(mods):
    lat = lattice_refs()
    check_lattice_facts(lat)
    rs = np.random.RandomState(21)
    colors = rs.rand(2, len(lat["ndc"]), 3).astype(np.float32)
    perm = rs.permutation(len(lat["faces"]))
    d = {"colors": colors, "perm": perm,
         "d_ndc": torch.from_numpy(np.stack([lat["ndc"]] * 2).astype(np.float32)).cuda(),
         "d_vz": torch.from_numpy(lat["vz"].astype(np.float32)).cuda(),
         "d_faces": torch.from_numpy(lat["faces"]).cuda(),
         "d_perm_faces": torch.from_numpy(lat["faces"][perm]).cuda(),
         "d_colors": torch.from_numpy(colors).cuda()}
    return dict(lat, **d)


@pytest.mark.parametrize("size", LATTICE_SIZES)
def test_lattice_owners_match_everywhere(mods, lattice, size):
    ops, _ = mods
    ptf, zbuf, bary, image = ops.rasterize_ndc(lattice["d_ndc"], lattice["d_vz"], lattice["d_faces"], size,
                                               znear=ZNEAR, colors=lattice["d_colors"], background=0.25)
    assert tuple(ptf.shape) == (2, size, size) and tuple(image.shape) == (2, 3, size, size)
    for m in range(2):
        ref = lattice["ref"][size][m]
        got, want = ptf[m].cpu().numpy(), ref["face"]
        assert np.array_equal(got, want), f"mesh {m}: owners differ at {np.argwhere(got != want)[:20].tolist()}"
        hit = want >= 0
        z, b = zbuf[m].cpu().numpy(), bary[m].cpu().numpy()
        assert (got[~hit] == -1).all() and (z[~hit] == -1).all() and (b[~hit] == -1).all()
        print(f"S={size} mesh {m}: covered {hit.mean():.3f}, z bit-equal to the oracle "
              f"{np.array_equal(z.astype(np.float64), ref['z'])}, bary bit-equal "
              f"{np.array_equal(b.astype(np.float64), ref['bary'])}")
        np.testing.assert_allclose(z[hit], ref["z"][hit], rtol=8 * EPS)
        np.testing.assert_allclose(b[hit], ref["bary"][hit], atol=8 * EPS)
        img = image64(ref, lattice["faces"], lattice["colors"][m].astype(np.float64), background=0.25)
        np.testing.assert_allclose(image[m].cpu().numpy(), img, rtol=0, atol=8 * EPS)
        assert (image[m].cpu().numpy()[:, ~hit] == np.float32(0.25)).all()


@pytest.mark.parametrize("size", LATTICE_SIZES)
def test_lattice_permuted_faces_give_the_same_picture(mods, lattice, size):
    ops, _ = mods
    perm = lattice["perm"]

    def run(faces):
        return ops.rasterize_ndc(lattice["d_ndc"], lattice["d_vz"], faces, size, znear=ZNEAR,
                                 colors=lattice["d_colors"], background=0.25)

    first, shuffled = run(lattice["d_faces"]), run(lattice["d_perm_faces"])
    assert torch.equal(shuffled[1], first[1]) and torch.equal(shuffled[3], first[3])  # zbuf, image: bit-equal
    for m in range(2):
        ref = lattice["ref"][size][m]
        a, b = first[0][m].cpu().numpy(), shuffled[0][m].cpu().numpy()
        assert ((a >= 0) == (b >= 0)).all()
        mapped = np.where(b >= 0, perm[np.maximum(b, 0)], -1)
        clear = ~ref["tie"]
        assert np.array_equal(mapped[clear], a[clear])  # no tie: the same face under its new index
        # a tie: the lowest NEW index among the tied faces, in the float64 arithmetic
        inverse = np.empty_like(perm)
        inverse[perm] = np.arange(len(perm))
        want = raster_np(lattice["ndc"], lattice["vz"][m], lattice["faces"], size, np.float64, rank=inverse)
        assert np.array_equal(mapped, want["face"]), f"mesh {m}: {(mapped != want['face']).sum()} owners differ"
        same = mapped == a
        print(f"S={size} mesh {m}: tie pixels {ref['tie'].mean():.3f}, another tied face owns {np.mean(~same):.3f}")
        b0, b1 = first[2][m].cpu().numpy(), shuffled[2][m].cpu().numpy()
        assert np.array_equal(b0[same], b1[same])  # bit-equal
        hit = b >= 0
        np.testing.assert_allclose(b1[hit], want["bary"][hit], rtol=0, atol=8 * EPS)  # the other face's corners


# ------------------------------------------------------------------ the real head against an owner search
def raster64_torch(ndc, vz, faces, size, znear=ZNEAR, chunk=128):
    """raster64 in plain torch float64 on the tensors' device, ``chunk`` faces
    at a time over all pixels: ndc [V, 2], vz [V] float64, faces [F, 3] int64.
    The same rules: the nearest depth, the lowest face among equal ones, the
    second-nearest depth and the edge tolerance for the ambiguity mask.
    Returns face [S, S] (int64), z, ambiguous (tensors)."""
    dev, f64 = ndc.device, torch.float64
    c = 1.0 - (2.0 * torch.arange(size, dtype=f64, device=dev) + 1.0) / size
    px, py = c.repeat(size)[None], c.repeat_interleave(size)[None]  # pixel p = i S + j
    npix = size * size
    inf = torch.tensor(float("inf"), dtype=f64, device=dev)
    best, second = inf.expand(npix).clone(), inf.expand(npix).clone()
    face = torch.full((npix,), -1, dtype=torch.int64, device=dev)
    edge_amb = torch.zeros(npix, dtype=torch.bool, device=dev)
    cols = torch.arange(npix, device=dev)
    tol = 1e-3 * 2.0 / size
    for f0 in range(0, faces.shape[0], chunk):
        fc = faces[f0:f0 + chunk]
        x, y, z = ndc[fc, 0], ndc[fc, 1], vz[fc]  # [C, 3]
        a = ((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0]))[:, None]
        valid = ~(z <= znear).any(1, keepdim=True) & ~(a == 0.0)
        sgn = torch.where(a > 0, 1.0, -1.0).to(f64)
        w, near, on_edge = [], None, None
        for p, q in ((1, 2), (2, 0), (0, 1)):
            dx, dy = (x[:, q] - x[:, p])[:, None], (y[:, q] - y[:, p])[:, None]
            wk = dx * (py - y[:, p, None]) - dy * (px - x[:, p, None])  # [C, P]
            w.append(wk)
            ln = torch.hypot(dx, dy)
            dist = torch.where(ln > 0, sgn * wk / ln, inf)
            near = (dist >= -tol) if near is None else near & (dist >= -tol)
            on_edge = (dist.abs() <= tol) if on_edge is None else on_edge | (dist.abs() <= tol)
        edge_amb |= (valid & near & on_edge).any(0)
        inside = valid & (sgn * w[0] >= 0) & (sgn * w[1] >= 0) & (sgn * w[2] >= 0)
        t = [w[k] / a / z[:, k, None] for k in range(3)]
        zz = torch.where(inside, 1.0 / (t[0] + t[1] + t[2]), inf)
        m1 = zz.min(0).values
        rows = torch.arange(zz.shape[0], device=dev)[:, None]
        first = torch.where(zz == m1[None], rows, zz.shape[0]).min(0).values.clamp_(max=zz.shape[0] - 1)
        zz[first, cols] = inf
        m2 = zz.min(0).values
        closer = m1 < best  # strict: equal depth keeps the lower face
        second = torch.minimum(torch.where(closer, best, m1), torch.minimum(second, m2))
        face = torch.where(closer, f0 + first, face)
        best = torch.where(closer, m1, best)
    hit = face >= 0
    depth_amb = hit & (second - best < 1e-4 * best)
    shape = (size, size)
    return {"face": face.reshape(shape), "z": torch.where(hit, best, -1.0).reshape(shape),
            "ambiguous": (edge_amb | depth_amb).reshape(shape)}


@pytest.mark.parametrize("size", (100, 256))
def test_two_heads_have_the_owners_of_a_float64_search(mods, topo_npz, size):
    """33 737 faces: 2109 groups, five rounds of the walk."""
    ops, rendering = mods
    verts = torch.from_numpy(recipe.load_meshes()["verts"][:2].astype(np.float32)).cuda()
    faces_np = np.asarray(topo_npz["face_0"], np.int32)
    faces = torch.from_numpy(faces_np).cuda()
    cam = rendering.look_at()
    ptf, zbuf, bary = ops.rasterize_meshes(verts, faces, cam, size)
    perm = np.random.RandomState(13).permutation(len(faces_np))
    d_perm = torch.from_numpy(perm).cuda()
    ptf_p, zbuf_p, bary_p = ops.rasterize_meshes(verts, torch.from_numpy(faces_np[perm]).cuda(), cam, size)
    assert torch.equal(zbuf_p, zbuf) and torch.equal(bary_p, bary)  # every group box is head-sized now
    view = verts.double() @ torch.from_numpy(cam.R).cuda() + torch.from_numpy(cam.T).cuda()
    for m in range(2):
        ref = raster64_torch(cam.scale * view[m, :, :2] / view[m, :, 2:3], view[m, :, 2].contiguous(), faces.long(),
                             size, znear=cam.znear)
        share, covered = ref["ambiguous"].double().mean().item(), (ref["face"] >= 0).double().mean().item()
        print(f"S={size} head {m}: ambiguous share {share:.4%}, covered {covered:.1%}")
        assert share <= 0.01  # the cap, on the oracle's own mask
        assert 0.25 <= covered <= 0.40
        clear = ~ref["ambiguous"]
        got = ptf[m].long()
        wrong = int((got[clear] != ref["face"][clear]).sum())
        assert wrong == 0, f"head {m}: {wrong} unambiguous pixels have another owner"
        rounds = torch.unique(got[clear & (got >= 0)] // (ROUND * GROUP)).tolist()
        print(f"  rounds with owners {rounds}")
        assert len(rounds) >= 4
        ok = clear & (got >= 0)
        dz = ((zbuf[m].double() - ref["z"])[ok].abs() / ref["z"][ok]).max().item()
        assert dz <= 1e-4  # the bound of the self-consistency test
        mapped = torch.where(ptf_p[m] >= 0, d_perm[ptf_p[m].long().clamp(min=0)], -1)
        assert torch.equal(mapped[clear], got[clear])


# ------------------------------------------------------------------ broadcast operands
def test_broadcast_colours_equal_the_expanded_batch(mods, scene):
    ops, rendering = mods
    size = 44
    dv, df, dc = scene["d_verts"], scene["d_faces"], scene["d_colors"]
    one = dc[:1].contiguous()
    wide = one.expand(3, -1, -1).contiguous()
    assert tuple(one.shape) == (1, dv.shape[1], 3) and wide.data_ptr() != one.data_ptr()
    ndc, vz, _ = ops.project_vertices(dv, scene["cam"])
    a = ops.rasterize_ndc(ndc, vz, df, size, colors=one, background=0.1)
    b = ops.rasterize_ndc(ndc, vz, df, size, colors=wide, background=0.1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    own = ops.rasterize_ndc(ndc, vz, df, size, colors=dc, background=0.1)
    assert torch.equal(a[3][0], own[3][0]) and not torch.equal(a[3][1], own[3][1])  # mesh 0's colours on every mesh
    ras = scene["ref"][size][1]
    flat = image64(ras, scene["faces"], scene["colors"][0].astype(np.float64), background=0.1)
    ok = ~ras["ambiguous"] & (ras["face"] >= 0)
    d = np.abs(a[3][1].cpu().numpy()[:, ok] - flat[:, ok]).max(0)
    assert (d <= 4 * bary_bound(ras, ok) + 1e-5).all()  # ... and they are the right ones
    ia = ops.interpolate_vertex_colors(a[0], a[2], df, one, background=0.1)
    ib = ops.interpolate_vertex_colors(a[0], a[2], df, wide, background=0.1)
    assert torch.equal(ia, ib) and torch.equal(ia, a[3])
    ca = ops.project_vertices(dv, scene["cam"], df, tex=one, shade=True)
    cb = ops.project_vertices(dv, scene["cam"], df, tex=wide, shade=True)
    for x, y in zip(ca, cb):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(ca[2]).all()) and not torch.equal(ca[2][0], ca[2][1])
    for shading in ("gouraud", "none"):
        ra = rendering.render(dv, df, one, shading=shading, image_size=size)
        rb = rendering.render(dv, df, wide, shading=shading, image_size=size)
        assert tuple(ra.shape) == (3, 3, size, size) and torch.equal(ra, rb)
        assert float(ra.max()) > 0.2


# ------------------------------------------------------------------ vertices that cannot be projected
def test_unprojectable_vertices_drop_their_faces_only(mods, scene):
    """One vertex of a sphere on the camera plane (view z = 0: x / 0), behind
    the camera, and NaN.  Its faces are dropped; the picture is the one of the
    mesh without them."""
    ops, rendering = mods
    size = 44
    cam = rendering.look_at(azim=0.0)  # R = diag(-1, 1, -1), T = (0, 0, 2.5): view z = 2.5 - z, exactly
    assert np.array_equal(np.abs(cam.R), np.eye(3)) and np.array_equal(cam.T, [0.0, 0.0, 2.5])
    base, faces = scene["verts"][0], scene["faces"]
    v = int(np.argmax(base[:-1, 2]))  # the vertex nearest to the camera: its faces are in the picture
    touch = (faces == v).any(1)
    assert 5 <= touch.sum() <= 6
    kept = np.flatnonzero(~touch)
    ndc, vz = cam.project(base.astype(np.float64))
    ref = raster64(ndc, vz, faces[kept], size, znear=cam.znear, crop=True)
    want = np.where(ref["face"] >= 0, kept[np.maximum(ref["face"], 0)], -1)
    whole = raster64(ndc, vz, faces, size, znear=cam.znear, crop=True)
    assert np.isin(whole["face"], np.flatnonzero(touch)).sum() >= 10  # they did own pixels
    share = ref["ambiguous"].mean()
    print(f"ambiguous share {share:.4%}, covered {np.mean(want >= 0):.1%}")
    assert share <= 0.01
    clear = ~ref["ambiguous"]
    verts = np.stack([base] * 3)
    verts[0, v, 2] = 2.5  # on the camera plane
    verts[1, v, 2] = 4.0  # behind the camera
    verts[2, v] = np.nan
    d_verts, d_faces = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    _, view_z, _ = ops.project_vertices(d_verts, cam)
    assert view_z[0, v].item() == 0.0 and view_z[1, v].item() == -1.5 and bool(torch.isnan(view_z[2, v]))
    ptf, zbuf, bary = ops.rasterize_meshes(d_verts, d_faces, cam, size)
    colors = torch.from_numpy(scene["colors"][0]).cuda()[None]
    image = rendering.render(d_verts, d_faces, colors, shading="none", image_size=size, camera=cam, background=0.25)
    torch.cuda.synchronize()
    flat = image64(ref, faces[kept], scene["colors"][0].astype(np.float64), background=0.25)
    ok = clear & (want >= 0)
    tol = 4 * bary_bound(ref, ok) + 1e-5
    for k in range(3):
        got = ptf[k].cpu().numpy()
        assert not np.isin(got, np.flatnonzero(touch)).any()  # the faces at that vertex own nothing
        assert np.array_equal(got[clear], want[clear]), f"case {k}: {(got[clear] != want[clear]).sum()} owners differ"
        assert bool(torch.isfinite(zbuf[k]).all()) and bool(torch.isfinite(bary[k]).all())
        assert bool(torch.isfinite(image[k]).all())
        assert got.min() == -1 and got.max() < len(faces)
        dz = np.abs(zbuf[k].cpu().numpy()[ok] - ref["z"][ok]) / ref["z"][ok]
        assert (dz <= 4 * bary_bound(ref, ok)).all()
        assert (np.abs(image[k].cpu().numpy()[:, ok] - flat[:, ok]).max(0) <= tol).all()
        bg = clear & (want < 0)
        assert (image[k].cpu().numpy()[:, bg] == np.float32(0.25)).all() and (zbuf[k].cpu().numpy()[bg] == -1).all()


# ------------------------------------------------------------------ a normal of valence 200
def normal_fan(n=200):
    """A fan of ``n`` faces about one apex (the last vertex), slightly off a
    plane; the apex is the first, the last or the middle corner of a face in
    turn (cyclic rotations: one orientation)."""
    rs = np.random.RandomState(11)
    ang = 2 * np.pi * (np.arange(n) + 0.3 * rs.rand(n)) / n
    rad = 0.8 + 0.4 * rs.rand(n)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.02 * rs.randn(n)], -1)
    verts = np.concatenate([rim, [[0.013, -0.007, 0.05]]]).astype(np.float32)
    i = np.arange(n)
    j = (i + 1) % n
    apex = np.full(n, n)
    corner = np.stack([np.stack([apex, i, j], -1), np.stack([i, j, apex], -1), np.stack([j, apex, i], -1)])
    return verts, corner[i % 3, i].astype(np.int32)


def normal_bound(verts, faces):
    """(valence + 8) eps sum |c_f| / |sum c_f| per vertex, from float64 cross
    products: each c_f is a few eps of |c_f| off, the running sum half an eps
    per step, and the normalisation divides by the sum's length."""
    v = verts.astype(np.float64)
    c = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    total, length, valence = np.zeros_like(v), np.zeros(len(v)), np.zeros(len(v))
    for k in range(3):
        np.add.at(total, faces[:, k], c)
        np.add.at(length, faces[:, k], np.linalg.norm(c, axis=1))
        np.add.at(valence, faces[:, k], 1)
    return (valence + 8) * EPS * length / np.linalg.norm(total, axis=1), valence


def test_vertex_normal_of_valence_200(mods):
    ops, _ = mods
    base, faces = normal_fan(200)
    verts = np.stack([base, base * np.float32(0.37) + np.float32(0.11)]).astype(np.float32)
    order = faces[:, 0] == 200, faces[:, 2] == 200
    assert order[0].sum() > 60 and order[1].sum() > 60  # the apex first, and last
    got = ops.vertex_normals(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()).cpu().numpy()
    for m in range(2):
        ref = normals64(verts[m].astype(np.float64), faces)
        bound, valence = normal_bound(verts[m], faces)
        assert valence[200] == 200 and (valence[:200] == 2).all()
        err = np.linalg.norm(got[m] - ref, axis=1)
        print(f"mesh {m}: apex error / bound {err[200] / bound[200]:.3g}, rim max {np.max(err[:200] / bound[:200]):.3g}")
        assert (err <= bound).all()
        assert abs(ref[200, 2]) > 0.9  # the fan is nearly flat: the apex normal is its axis
