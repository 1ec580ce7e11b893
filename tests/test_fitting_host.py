"""CPU tests of the latent-fitting host side: the Procrustes alignment, the
argument validation of the two Chamfer entry points (before any HIP call) and
the parameter-freezing context of the fit loop.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, fitting, ops  # noqa: E402


def _rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_procrustes_recovers_similarity():
    """scan = s * template . Q + t (Q a proper rotation): the alignment maps
    the scan's points and landmarks back onto the template's to 1e-6."""
    rs = np.random.RandomState(3)
    tpl_lnd = rs.randn(7, 3) * 40 + np.array([3.0, -120.0, 55.0])
    tpl_pts = rs.randn(500, 3) * 60 + np.array([3.0, -120.0, 55.0])
    rot, s, t = _rotation(rs), 0.37, np.array([250.0, 10.0, -90.0])
    assert np.linalg.det(rot) > 0
    pts, lnd = fitting.procrustes_align(s * tpl_lnd @ rot + t, tpl_lnd, s * tpl_pts @ rot + t)
    assert pts.shape == (500, 3) and lnd.shape == (7, 3)
    assert np.abs(pts - tpl_pts).max() <= 1e-6
    assert np.abs(lnd - tpl_lnd).max() <= 1e-6


def test_procrustes_allows_reflections():
    """The stated convention (scipy's orthogonal_procrustes, as the reference
    calls it): the orthogonal factor may have det -1, so a MIRRORED scan is
    mapped back exactly too -- not to the best proper rotation."""
    rs = np.random.RandomState(4)
    tpl_lnd = rs.randn(6, 3) * 30
    tpl_pts = rs.randn(200, 3) * 30
    mirror = _rotation(rs) @ np.diag([1.0, 1.0, -1.0])
    assert np.linalg.det(mirror) < 0
    pts, lnd = fitting.procrustes_align(2.5 * tpl_lnd @ mirror + 7.0, tpl_lnd, 2.5 * tpl_pts @ mirror + 7.0)
    assert np.abs(pts - tpl_pts).max() <= 1e-6
    assert np.abs(lnd - tpl_lnd).max() <= 1e-6


def test_procrustes_noisy_landmarks_scale_is_singular_value_sum():
    """With landmarks that are no exact similarity image, the scale is the sum
    of the singular values of A^T B (< 1 for unit-norm A, B) and the mapped
    landmarks are the least-squares fit, not an exact match."""
    rs = np.random.RandomState(5)
    dst = rs.randn(8, 3)
    src = dst @ _rotation(rs) * 3.0 + rs.randn(8, 3) * 0.05
    _, lnd = fitting.procrustes_align(src, dst, src)
    a = (dst - dst.mean(0)) / np.linalg.norm(dst - dst.mean(0))
    b = (src - src.mean(0)) / np.linalg.norm(src - src.mean(0))
    u, w, vt = np.linalg.svd(a.T @ b)
    assert w.sum() < 1.0
    expect = (b @ (u @ vt).T) * w.sum() * np.linalg.norm(dst - dst.mean(0)) + dst.mean(0)
    np.testing.assert_allclose(lnd, expect, atol=1e-12)
    assert 1e-4 < np.abs(lnd - dst).max() < 0.2


def test_procrustes_rejects_bad_shapes():
    with pytest.raises(ValueError):
        fitting.procrustes_align(np.zeros((4, 3)), np.zeros((5, 3)), np.zeros((9, 3)))
    with pytest.raises(ValueError):
        fitting.procrustes_align(np.ones((4, 3)), np.ones((4, 3)), np.zeros((9, 3)))  # single point


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def test_chamfer_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 13
    rc = lib.cfsd_nn_points(None, None, None, None, None, 0, 1, 1, 1, 4, 4, None)
    assert rc == -1 and b"null" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_points(p, p, p, p, None, 0, 2, 2, 1, 0, 4, None)  # N = 0
    assert rc == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_points(p, p, p, p, None, 0, 2, 2, 1, 4, 0, None)  # P = 0
    assert rc == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_points(p, p, p, p, None, 0, 4, 2, 1, 4, 4, None)  # batch 2 against 4
    assert rc == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()
    rc = lib.cfsd_chamfer_bwd(None, None, None, None, None, None, None, None, 1, 1, 4, 4, None)
    assert rc == -1 and b"null" in lib.cfsd_last_error_string()
    rc = lib.cfsd_chamfer_bwd(p, p, p, p, p, p, p, p, 2, 1, 0, 4, None)
    assert rc == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    rc = lib.cfsd_chamfer_bwd(p, p, p, p, p, p, p, p, 2, 1, 4, 0, None)
    assert rc == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    # the segment workspace is a function of the shapes: none for a short
    # reference set, winners of every segment for a long one
    assert lib.cfsd_nn_points_workspace(16, 257, 2 * ops.NN_TILE + 3) == 0
    assert lib.cfsd_nn_points_workspace(1, 65, 300) == 2 * 65 * 8
    assert lib.cfsd_nn_points_workspace(0, 65, 300) == 0
    # a cut reference set without its workspace is refused (rc -2), not run
    rc = lib.cfsd_nn_points(p, p, p, p, None, 0, 1, 1, 1, 65, 300, None)
    assert rc == -2 and b"workspace" in lib.cfsd_last_error_string()


def test_ops_tile_matches_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cfsd.h")).read()
    assert f"#define CFSD_NN_TILE {ops.NN_TILE}\n" in src


def test_chamfer_distance_rejects_unsupported_options():
    x, y = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    for kw in ({"x_normals": x}, {"y_normals": y}, {"x_lengths": torch.tensor([4])},
               {"y_lengths": torch.tensor([5])}, {"norm": 1}, {"weights": torch.ones(1)},
               {"batch_reduction": "max"}, {"point_reduction": None}):
        with pytest.raises(ValueError):
            ops.chamfer_distance(x, y, **kw)
    with pytest.raises(ValueError):  # host tensors never reach a kernel
        ops.chamfer_distance(x, y)


def test_frozen_restores_flags_and_modes_exactly():
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Sequential(torch.nn.Linear(4, 2)))
    net[0].bias.requires_grad_(False)
    net.train()
    net[1].eval()
    flags = [p.requires_grad for p in net.parameters()]
    modes = [m.training for m in net.modules()]
    with pytest.raises(RuntimeError):
        with fitting.frozen(net):
            assert not any(p.requires_grad for p in net.parameters())
            net.train()  # what generate_for_opt does inside the loop
            raise RuntimeError("boom")
    assert [p.requires_grad for p in net.parameters()] == flags
    assert [m.training for m in net.modules()] == modes
    with fitting.frozen(None):
        pass
