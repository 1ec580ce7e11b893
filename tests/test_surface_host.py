"""CPU tests of the surface-fitting host side: argument validation of the two
point-to-triangle entry points (before any HIP call), the OBJ face reader,
the vertex path of the fit loop staying clear of the surface operators, and
the float64 oracle of tests/test_gpu_surface.py against dense barycentric
sampling.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, data, fitting, ops  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def test_point_face_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(256)
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 14
    big = 1 << 20

    def fwd(points=p, verts=p, faces=p, out=p, ws=p, nbytes=big, batch=2, bp=2, bv=1, n=4, nv=5, nf=6, flags=1):
        return lib.cfsd_point_face(points, verts, faces, None, out, out, out, None, ws, nbytes, batch, bp, bv, n, nv,
                                   nf, flags, None)

    for kw in ({"points": None}, {"verts": None}, {"faces": None}, {"out": None}):
        assert fwd(**kw) == -1 and b"null" in lib.cfsd_last_error_string()
    for kw in ({"batch": 0}, {"n": 0}, {"nv": 0}, {"nf": 0}):
        assert fwd(**kw) == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    assert fwd(batch=4, bp=2, bv=1) == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()
    assert fwd(batch=4, bp=4, bv=3) == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()
    assert fwd(batch=1 << 12, bp=1 << 12, n=1 << 18) == -1 and b"2^31" in lib.cfsd_last_error_string()
    assert fwd(flags=4) == -1 and b"flags" in lib.cfsd_last_error_string()
    # the workspace is always needed: records of every face + one sphere per group
    need = lib.cfsd_point_face_workspace(1, 6)
    assert need == 6 * 64 + 1 * 16
    assert lib.cfsd_point_face_workspace(3, 2 * ops.PF_GROUP + 1) == 3 * ((2 * ops.PF_GROUP + 1) * 64 + 3 * 16)
    assert lib.cfsd_point_face_workspace(0, 6) == 0 and lib.cfsd_point_face_workspace(1, 0) == 0
    assert fwd(ws=None, nbytes=0) == -2 and b"workspace" in lib.cfsd_last_error_string()
    assert fwd(nbytes=need - 1) == -2 and b"workspace" in lib.cfsd_last_error_string()
    assert fwd(ws=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.cfsd_last_error_string()

    def bwd(points=p, gp=p, seg=p, gv=p, batch=2, bp=2, bv=1, n=4, nv=5, nf=6):
        return lib.cfsd_point_face_bwd(points, p, p, p, p, p, gp, seg, seg, gv, batch, bp, bv, n, nv, nf, None)

    assert bwd(points=None) == -1 and b"null" in lib.cfsd_last_error_string()
    assert bwd(gp=None) == -1 and b"null" in lib.cfsd_last_error_string()
    assert bwd(seg=None) == -1 and b"null" in lib.cfsd_last_error_string()  # vertex gradient without its runs
    assert bwd(n=0) == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    assert bwd(nf=0) == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    assert bwd(batch=4, bp=2) == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()


def test_ops_constants_match_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cfsd.h")).read()
    assert f"#define CFSD_PF_GROUP {ops.PF_GROUP}\n" in src
    assert f"#define CFSD_PF_CULL {ops.PF_CULL}\n" in src
    assert f"#define CFSD_PF_PREPARED {ops.PF_PREPARED}\n" in src


def test_surface_operators_refuse_host_tensors_and_bad_faces():
    pts, verts = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for fn in (ops.point_face_distance, ops.point_mesh_distance):
        with pytest.raises(ValueError):  # host tensors never reach a kernel
            fn(pts, verts, faces)
    with pytest.raises(ValueError):
        ops.surface_distance(verts, faces, pts, faces)
    with pytest.raises(ValueError):
        ops.surface_distance(verts, faces, pts, faces, batch_reduction="max")
    with pytest.raises(ValueError):
        ops.face_table(faces.long(), 5)  # dtype
    with pytest.raises(ValueError):
        ops.face_table(np.zeros((1, 3), np.int32), 5)


OBJ = """# every f form, a quad and a negative index
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
f 1 2 3
f 1/1 3/1 4/1
f 1/1/1 2/1/1 4/1/1
f 2//1 3//1 4//1
v 0 0 1
f 1 2 3 4
f -1 -5 -4
f 5 1 2 3 4
"""


def test_read_obj_faces(tmp_path):
    path = tmp_path / "scan.obj"
    path.write_text(OBJ)
    faces = data.read_obj_faces(str(path))
    assert faces.dtype == np.int64
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3],
                              [0, 1, 2], [0, 2, 3],            # the quad as a fan
                              [4, 0, 1],                       # -1 = the fifth vertex, -5 = the first
                              [4, 0, 1], [4, 1, 2], [4, 2, 3]]  # a pentagon
    assert data.read_obj_faces(str(path), n_verts=5).shape == (10, 3)
    with pytest.raises(ValueError):
        data.read_obj_faces(str(path), n_verts=4)
    assert len(data.read_obj_vertices(str(path))) == 5
    (tmp_path / "bad.obj").write_text("v 0 0 0\nf 0 1 1\n")
    with pytest.raises(ValueError):
        data.read_obj_faces(str(tmp_path / "bad.obj"))
    (tmp_path / "none.obj").write_text("v 0 0 0\n")
    assert data.read_obj_faces(str(tmp_path / "none.obj")).shape == (0, 3)


def test_fit_points_without_faces_never_reaches_a_surface_operator(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a surface operator was reached on the vertex path")

    for name in ("surface_distance", "point_mesh_distance", "point_face_distance", "point_face_bwd", "SurfaceMesh",
                 "face_table"):
        assert hasattr(ops, name)
        monkeypatch.setattr(ops, name, boom)
    calls = []

    def chamfer(x, y, batch_reduction="mean", **kw):
        calls.append(batch_reduction)
        d = ((x[:, :, None] - y[:, None]) ** 2).sum(-1)
        per = d.min(2).values.mean(1) + d.min(1).values.mean(1)
        return (per if batch_reduction is None else per.mean()), None

    monkeypatch.setattr(ops, "chamfer_distance", chamfer)
    net = torch.nn.Linear(4, 18)
    res = fitting.fit_points(lambda z: net(z).reshape(-1, 6, 3), torch.randn(9, 3), torch.randn(2, 3), [0, 4], None,
                             None, torch.zeros(4), n_starts=3, iterations=2, module=net)
    assert calls == ["mean", "mean", None]
    assert res.surface_mm is None and res.errors_shape.shape == (3,)
    with pytest.raises(ValueError):  # the two face tensors go together
        fitting.fit_points(lambda z: net(z).reshape(-1, 6, 3), torch.randn(9, 3), torch.randn(2, 3), [0, 4], None,
                           None, torch.zeros(4), n_starts=3, iterations=2, module=net,
                           target_faces=torch.zeros(1, 3, dtype=torch.int32))


def test_oracle_agrees_with_dense_barycentric_sampling():
    """The float64 oracle of the GPU tests against the minimum over a dense
    barycentric grid of each triangle: the grid's nearest sample is within one
    step (in every weight) of the true nearest point, so
    0 <= d_grid - d_oracle <= step * longest edge, squared distances compared
    through their roots."""
    from test_gpu_surface import tri_closest64

    rs = np.random.RandomState(0)
    m = 200
    i, j = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    keep = i + j <= m
    wv, ww = torch.from_numpy(i[keep] / m), torch.from_numpy(j[keep] / m)
    grid_w = torch.stack([1 - wv - ww, wv, ww], -1)  # [S, 3]
    tris = [rs.randn(3, 3) for _ in range(4)]
    tris.append(np.array([[0.0, 0, 0], [2, 0, 0], [1, 0, 0]]))        # collinear: a segment
    tris.append(np.array([[1.0, 2, 3], [1, 2, 3], [1, 2, 3]]))        # a point
    tris.append(np.array([[0.0, 0, 0], [1, 0, 0], [0.5, 1e-3, 0]]))   # a sliver
    for t in tris:
        tri = torch.from_numpy(t)
        pts = torch.from_numpy(np.concatenate([rs.randn(60, 3) * 2, t.mean(0) + rs.randn(40, 3) * 0.2]))
        d2, w = tri_closest64(pts, tri[0], tri[1], tri[2])
        samples = grid_w @ tri  # [S, 3]
        d_grid = ((pts[:, None] - samples[None]) ** 2).sum(-1).min(1).values.sqrt()
        d = d2.sqrt()
        edge = max(np.linalg.norm(t[a] - t[b]) for a, b in ((0, 1), (1, 2), (2, 0)))
        assert bool((d <= d_grid + 1e-12).all()), "a sample of the triangle is nearer than the oracle's nearest point"
        assert bool((d_grid - d <= 2 * edge / m + 1e-12).all())
        # the weights are a point of the triangle and rebuild the distance
        assert float(w.min()) >= -1e-12 and (w.sum(-1) - 1).abs().max().item() <= 1e-12
        rebuilt = ((pts - w @ tri) ** 2).sum(-1)
        assert (rebuilt - d2).abs().max().item() <= 1e-12 * (1 + d2.max().item())
