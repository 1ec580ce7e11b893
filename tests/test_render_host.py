"""CPU tests of the rendering host side: the camera against its closed form,
argument validation of the rendering entry points (before any HIP call), the
header constants, the operators' refusal of host tensors, the PNG writer, the
image grid and the error colour map.  No kernel is launched."""
import ctypes
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, ops, rendering  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


# ------------------------------------------------------------------ camera
def closed_form(dist, elev, azim):
    """The specification, written out independently of rendering.Camera."""
    e, a = math.radians(elev), math.radians(azim)
    c = np.array([dist * math.cos(e) * math.sin(a), dist * math.sin(e), dist * math.cos(e) * math.cos(a)])
    z = -c / math.sqrt(float(c @ c))
    up = np.array([0.0, 1.0, 0.0])
    x = np.array([up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]])
    x = x / math.sqrt(float(x @ x))
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]])
    r = np.zeros((3, 3))
    r[:, 0], r[:, 1], r[:, 2] = x, y, z
    return c, r, -(c @ r)


@pytest.mark.parametrize("dist,elev,azim", [(2.5, 0.0, 15.0), (3.0, 20.0, -40.0)])
def test_look_at_matches_closed_form(dist, elev, azim):
    cam = rendering.look_at(dist, elev, azim)
    c, r, t = closed_form(dist, elev, azim)
    np.testing.assert_allclose(cam.R, r, atol=1e-15)
    np.testing.assert_allclose(cam.T, t, atol=1e-15)
    np.testing.assert_allclose(cam.centre, c, atol=1e-15)
    np.testing.assert_allclose(cam.R.T @ cam.R, np.eye(3), atol=1e-15)  # orthonormal
    assert np.linalg.det(cam.R) == pytest.approx(1.0, abs=1e-14)
    xy, z = cam.project(np.zeros(3))  # the origin: the image centre, at depth dist
    np.testing.assert_allclose(xy, 0.0, atol=1e-15)
    assert z == pytest.approx(dist, abs=1e-14)
    assert cam.scale == pytest.approx(1 / math.tan(math.radians(30)), rel=1e-15) and cam.znear == 1.0
    p = cam.params
    assert p.dtype == np.float32 and p.shape == (14,)
    np.testing.assert_array_equal(p[:9].reshape(3, 3), cam.R.astype(np.float32))
    np.testing.assert_array_equal(p[9:12], cam.T.astype(np.float32))
    assert p[12] == np.float32(cam.scale) and p[13] == 1.0


def test_default_camera_orientation():
    """At the default view NDC +Y is world up and +X points to the LEFT of the image."""
    cam = rendering.look_at()
    assert (cam.dist, cam.elev, cam.azim, cam.fov) == (2.5, 0.0, 15.0, 60.0)
    up, _ = cam.project(np.array([0.0, 0.1, 0.0]))
    assert up[1] > 0 and abs(up[0]) < 1e-15
    # seen from the front (the camera near +z) world +x is on the viewer's right: NDC -x, a higher pixel column
    side, _ = cam.project(np.array([0.1, 0.0, 0.0]))
    assert side[0] < 0 and abs(side[1]) < 1e-15


# ------------------------------------------------------------------ entry points
def test_render_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(256)
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 15
    err = lib.cfsd_last_error_string
    big = 1 << 24

    def normals(verts=p, faces=p, vp=p, vi=p, out=p, batch=2, nv=5, nf=6):
        return lib.cfsd_vertex_normals(verts, faces, vp, vi, out, batch, nv, nf, None)

    for kw in ({"verts": None}, {"faces": None}, {"vp": None}, {"vi": None}, {"out": None}):
        assert normals(**kw) == -1 and b"null" in err()
    for kw in ({"batch": 0}, {"nv": 0}, {"nf": 0}, {"batch": -1}):
        assert normals(**kw) == -1 and b"bad sizes" in err()
    assert normals(batch=1 << 12, nv=1 << 18) == -1 and b"2^31" in err()
    assert normals(batch=1 << 12, nf=1 << 16) == -1 and b"2^31" in err()

    def vertices(verts=p, cam=p, faces=p, vp=p, vi=p, tex=p, ndc=p, vz=p, colors=p, batch=2, bt=2, nv=5, nf=6):
        return lib.cfsd_render_vertices(verts, cam, faces, vp, vi, tex, ndc, vz, colors, batch, bt, nv, nf, 0.0, 0.0,
                                        3.0, 0.5, 1.0, 0.2, 0.5, 0.5, None)

    for kw in ({"verts": None}, {"cam": None}, {"ndc": None}, {"vz": None}):
        assert vertices(**kw) == -1 and b"null" in err()
    for kw in ({"faces": None}, {"vp": None}, {"vi": None}):  # colours need the faces and their runs
        assert vertices(**kw) == -1 and b"null" in err()
    for kw in ({"batch": 0}, {"nv": 0}, {"nf": 0}):
        assert vertices(**kw) == -1 and b"bad sizes" in err()
    assert vertices(batch=4, bt=3) == -1 and b"must be 1 or 4" in err()
    assert vertices(batch=1 << 12, nv=1 << 18) == -1 and b"2^31" in err()

    need = lib.cfsd_raster_workspace(2, 6)
    assert need == 2 * (6 * 48 + 1 * 16)
    assert lib.cfsd_raster_workspace(3, 2 * ops.RN_GROUP + 1) == 3 * ((2 * ops.RN_GROUP + 1) * 48 + 3 * 16)
    assert lib.cfsd_raster_workspace(0, 6) == 0 and lib.cfsd_raster_workspace(1, 0) == 0
    assert lib.cfsd_raster_workspace(1 << 12, 1 << 16) == 0

    def raster(ndc=p, vz=p, faces=p, colors=p, ptf=p, zbuf=p, bary=p, image=p, ws=p, nbytes=big, batch=2, bc=2,
               nv=5, nf=6, size=16):
        return lib.cfsd_rasterize(ndc, vz, faces, colors, ptf, zbuf, bary, image, ws, nbytes, batch, bc, nv, nf, size,
                                  1.0, 0.0, 0.0, 0.0, None)

    for kw in ({"ndc": None}, {"vz": None}, {"faces": None}, {"ptf": None}, {"zbuf": None}, {"bary": None}):
        assert raster(**kw) == -1 and b"null" in err()
    for kw in ({"colors": None}, {"image": None}):  # they go together
        assert raster(**kw) == -1 and b"null" in err()
    for kw in ({"batch": 0}, {"nv": 0}, {"nf": 0}, {"size": 0}, {"size": -3}, {"size": ops.RN_MAX_SIZE + 1}):
        assert raster(**kw) == -1 and b"bad sizes" in err()
    assert raster(batch=4, bc=2) == -1 and b"must be 1 or 4" in err()
    assert raster(batch=64, bc=64, size=4096) == -1 and b"2^31" in err()  # 64 x 4096^2 x 3
    assert raster(batch=1 << 12, bc=1, nf=1 << 16) == -1 and b"2^31" in err()
    assert raster(ws=None, nbytes=0) == -2 and b"workspace" in err()
    assert raster(nbytes=need - 1) == -2 and b"workspace" in err()
    assert raster(ws=ctypes.c_void_p(260)) == -1 and b"aligned" in err()

    def interp(ptf=p, bary=p, faces=p, colors=p, image=p, batch=2, bc=1, nv=5, nf=6, size=16):
        return lib.cfsd_interpolate_colors(ptf, bary, faces, colors, image, batch, bc, nv, nf, size, 0.0, 0.0, 0.0,
                                           None)

    for kw in ({"ptf": None}, {"bary": None}, {"faces": None}, {"colors": None}, {"image": None}):
        assert interp(**kw) == -1 and b"null" in err()
    for kw in ({"batch": 0}, {"nv": 0}, {"nf": 0}, {"size": 0}, {"size": 4097}):
        assert interp(**kw) == -1 and b"bad sizes" in err()
    assert interp(batch=4, bc=3) == -1 and b"must be 1 or 4" in err()
    assert interp(batch=64, bc=64, size=4096) == -1 and b"2^31" in err()


def test_render_constants_match_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cfsd.h")).read()
    assert f"#define CFSD_RN_GROUP {ops.RN_GROUP}\n" in src
    assert f"#define CFSD_RN_MAX_SIZE {ops.RN_MAX_SIZE}\n" in src


def test_render_operators_refuse_host_tensors_and_bad_faces():
    verts = torch.zeros(1, 5, 3)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cam = rendering.look_at()
    with pytest.raises(ValueError):
        ops.vertex_normals(verts, faces)
    with pytest.raises(ValueError):
        ops.rasterize_ndc(torch.zeros(1, 5, 2), torch.ones(1, 5), faces, 16)
    with pytest.raises(ValueError):
        ops.rasterize_meshes(verts, faces, cam, 16)
    with pytest.raises(ValueError):
        ops.interpolate_vertex_colors(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, 3), faces,
                                      torch.zeros(1, 5, 3))
    with pytest.raises(ValueError):
        rendering.render(verts, faces)
    with pytest.raises(ValueError):
        rendering.gouraud_colors(verts, faces)
    with pytest.raises(ValueError):
        ops.render_faces(faces.long(), 5)  # dtype
    with pytest.raises(ValueError):
        ops.render_faces(np.zeros((1, 3), np.int32), 5)
    with pytest.raises(ValueError):
        rendering.render(verts, faces, shading="phong")
    with pytest.raises(ValueError):
        rendering.render(verts, faces, shading="none")  # no colours to show
    for bad in (0, 4097, 16.5):
        with pytest.raises(ValueError):
            ops._image_size(bad)


# ------------------------------------------------------------------ PNG
def decode_png(path):
    """(width, height, [H, W, 3] uint8) of an 8-bit RGB PNG whose rows use filter 0; checks every CRC."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [c[0] for c in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    data = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    rows = np.frombuffer(data, np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return w, h, rows[:, 1:].reshape(h, w, 3)


def test_save_png_round_trip(tmp_path):
    rs = np.random.RandomState(0)
    img = torch.from_numpy(rs.rand(3, 7, 11).astype(np.float32))
    img[:, 0, 0] = torch.tensor([-0.5, 1.5, 0.5])  # clamped only here
    img[:, 0, 1] = torch.tensor([0.0, 1.0, 0.49999 / 255])
    path = rendering.save_png(str(tmp_path / "a.png"), img)
    w, h, rgb = decode_png(path)
    assert (w, h) == (11, 7)
    want = np.floor(np.clip(img.numpy().astype(np.float32), 0, 1) * np.float32(255) + np.float32(0.5))
    np.testing.assert_array_equal(rgb, want.astype(np.uint8).transpose(1, 2, 0))
    assert rgb[0, 0].tolist() == [0, 255, 128] and rgb[0, 1].tolist() == [0, 255, 0]
    u8 = torch.from_numpy(rs.randint(0, 256, (3, 4, 5)).astype(np.uint8))
    _, _, back = decode_png(rendering.save_png(str(tmp_path / "b.png"), u8))
    np.testing.assert_array_equal(back, u8.numpy().transpose(1, 2, 0))
    with pytest.raises(ValueError):
        rendering.save_png(str(tmp_path / "c.png"), torch.zeros(4, 4))
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (11, 7)
        np.testing.assert_array_equal(np.asarray(im), rgb)


# ------------------------------------------------------------------ grid
def test_make_grid_geometry():
    imgs = torch.arange(5, dtype=torch.float32).reshape(5, 1, 1, 1).expand(5, 3, 6, 9) * 0.1
    g = rendering.make_grid(imgs, nrow=4, padding=10, pad_value=1.0)
    assert tuple(g.shape) == (3, 2 * 16 + 10, 4 * 19 + 10)
    mask = torch.zeros(g.shape[1:], dtype=torch.bool)
    for k in range(5):
        y, x = divmod(k, 4)
        cell = g[:, y * 16 + 10:y * 16 + 16, x * 19 + 10:x * 19 + 19]
        assert torch.equal(cell, imgs[k])
        mask[y * 16 + 10:y * 16 + 16, x * 19 + 10:x * 19 + 19] = True
    assert bool((g[:, ~mask] == 1.0).all())  # the frame and the three empty cells
    one = rendering.make_grid(imgs[:2], nrow=4, padding=2, pad_value=0.25)  # fewer images than a row
    assert tuple(one.shape) == (3, 6 + 4, 2 * 11 + 2)
    assert one[0, 0, 0] == 0.25 and torch.equal(one[:, 2:8, 13:22], imgs[1])


# ------------------------------------------------------------------ colours
def test_plasma_table_is_matplotlibs():
    tab = rendering.plasma_table()
    assert tab.shape == (256, 3) and tab.dtype == np.uint8
    assert tab[0].tolist() == [12, 7, 134] and tab[255].tolist() == [239, 248, 33]  # plasma's published ends
    matplotlib = pytest.importorskip("matplotlib")
    ref = matplotlib.colormaps["plasma"](np.arange(256), bytes=True)[:, :3]
    np.testing.assert_array_equal(tab, ref)


def test_errors_to_colors_index_rule():
    tab = rendering.plasma_table().astype(np.float32) / np.float32(255)
    e = torch.tensor([0.0, 2.0 * (1 / 256 - 1e-6), 2.0 / 256, 1.0, 2.0 - 1e-6, 2.0, 7.0, -1.0])
    got = rendering.errors_to_colors(e, 0, 2.0).numpy()
    assert got.shape == (8, 3) and got.dtype == np.float32
    np.testing.assert_array_equal(got, tab[[0, 0, 1, 128, 255, 255, 255, 0]])
    same = rendering.errors_to_colors(torch.tensor([[0.5, 1.0], [1.5, 1.0]]), 1.0, 1.0).numpy()  # min == max
    assert same.shape == (2, 2, 3)
    np.testing.assert_array_equal(same, tab[[[0, 0], [255, 0]]])
    auto = rendering.errors_to_colors(torch.tensor([1.0, 3.0, 2.0])).numpy()  # range from the data
    np.testing.assert_array_equal(auto, tab[[0, 255, 128]])
    with pytest.raises(ValueError):
        rendering.errors_to_colors(e, 0, 1, cmap="viridis")


# ------------------------------------------------------------------ the GPU suite's oracle and scenes
def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _sphere_at_48():
    from test_gpu_render import SCALES, SHIFT, icosphere
    v, faces = icosphere(2)
    v = (v * np.asarray(SCALES[0]) + np.asarray(SHIFT)).astype(np.float32).astype(np.float64)
    ndc, vz = rendering.look_at().project(v)
    return ndc, vz, faces


def test_raster64_crop_changes_nothing():
    """The oracle's per-face pass over the face's pixel box grown by two
    pixels gives what the pass over the whole image gives, field by field."""
    from test_gpu_render import exact_scene, raster64
    ndc, vz, faces = exact_scene()
    _same(raster64(ndc, vz, faces, 16), raster64(ndc, vz, faces, 16, crop=True))
    ndc, vz, faces = _sphere_at_48()
    whole = raster64(ndc, vz, faces, 48)
    assert 0.2 < np.mean(whole["face"] >= 0) < 0.9 and whole["ambiguous"].any()
    _same(whole, raster64(ndc, vz, faces, 48, crop=True))


def test_torch_owner_search_is_raster64():
    """The chunked torch restatement of the oracle (the real head's owner
    search on the GPU) against raster64, on the CPU: the same owners, the
    same ambiguity mask, the same depths; with a chunk that splits the list."""
    from test_gpu_render import exact_scene, raster64
    from test_gpu_render_walk import raster64_torch
    for (ndc, vz, faces), size in ((exact_scene(), 16), (_sphere_at_48(), 48)):
        ref = raster64(ndc, vz, faces, size)
        for chunk in (7, 128):
            got = raster64_torch(torch.from_numpy(ndc), torch.from_numpy(vz), torch.from_numpy(faces).long(), size,
                                 chunk=chunk)
            assert np.array_equal(got["face"].numpy(), ref["face"])
            assert np.array_equal(got["ambiguous"].numpy(), ref["ambiguous"])
            np.testing.assert_allclose(got["z"].numpy(), ref["z"], rtol=1e-14)


def test_lattice_scene_is_exact_in_float32():
    """The two-round lattice of test_gpu_render_walk.py: the float32
    restatement of the kernel's arithmetic gives the float64 oracle's owners,
    depths and weights at every pixel of both meshes at every size, bit for
    bit, and the oracle shows what the scene is built to show."""
    from test_gpu_render_walk import LATTICE_SIZES, check_lattice_facts, lattice_refs, raster_np
    lat = lattice_refs()
    check_lattice_facts(lat)
    for size in LATTICE_SIZES:
        for m in range(2):
            ref = lat["ref"][size][m]
            for dtype in (np.float32, np.float64):
                got = raster_np(lat["ndc"], lat["vz"][m], lat["faces"], size, dtype)
                assert np.array_equal(got["face"], ref["face"]), (size, m, dtype)
                assert np.array_equal(got["z"].astype(np.float64), ref["z"])
                assert np.array_equal(got["bary"].astype(np.float64), ref["bary"])
