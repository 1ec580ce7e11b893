"""CPU tests of the uniform-grid nearest-neighbour search's host side: the ABI
(version, entry points read from cfsd.h), the argument validation of the C
entry points before any HIP call, the ValueErrors of the Python layer and the
default cell rule.  No kernel is launched."""
import ctypes
import os

import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, fitting, ops  # noqa: E402

NEW = ("cfsd_nn_grid_build_workspace", "cfsd_nn_grid_build", "cfsd_nn_points_grid")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def test_abi_version_and_entry_points(lib):
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 24
    for name in NEW:
        assert name in _abi.SIGNATURES, f"{name} is not declared in cfsd.h"
        assert hasattr(lib, name), f"libcfsd.so does not export {name}"
    assert _abi.SIGNATURES["cfsd_nn_grid_build_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert len(_abi.SIGNATURES["cfsd_nn_points_grid"][1]) == 16
    assert ops.NN_GRID_MAX == _abi.CONSTANTS["CFSD_NN_GRID_MAX"] == 128


def test_grid_workspace_is_a_function_of_the_shapes(lib):
    ws = lib.cfsd_nn_grid_build_workspace

    def expect(br, p, cells):
        pad = lambda v: (v + 15) // 16 * 16  # noqa: E731
        return br * p * 16 + br * 16 * 4 + pad(br * (cells + 1) * 4) + pad(br * p * 4)

    assert ws(1, 1, 1, 1, 1) == expect(1, 1, 1)
    assert ws(16, 300, 6, 6, 6) == expect(16, 300, 216)
    assert ws(3, 17, 1, 7, 128) == expect(3, 17, 7 * 128)
    for bad in ((0, 5, 2, 2, 2), (1, 0, 2, 2, 2), (1, 5, 0, 2, 2), (1, 5, 2, 129, 2), (1, 5, 2, 2, -1)):
        assert ws(*bad) == 0


def test_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)
    big = ctypes.c_size_t(1 << 30)
    rc = lib.cfsd_nn_grid_build(None, None, big, 0, None, None, 1, 4, 2, 2, 2, None)
    assert rc == -1 and b"null" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_grid_build(p, p, big, 0, None, None, 1, 0, 2, 2, 2, None)
    assert rc == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    for cells in ((0, 2, 2), (2, 129, 2), (2, 2, -3)):
        rc = lib.cfsd_nn_grid_build(p, p, big, 0, None, None, 1, 4, *cells, None)
        assert rc == -1 and b"outside 1..128" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_grid_build(p, p, ctypes.c_size_t(8), 0, None, None, 1, 4, 2, 2, 2, None)
    assert rc == -2 and b"grid buffer" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_grid_build(p, ctypes.c_void_p(20), big, 0, None, None, 1, 4, 2, 2, 2, None)
    assert rc == -1 and b"aligned" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_grid_build(p, p, big, 7, None, None, 1, 4, 2, 2, 2, None)
    assert rc == -1 and b"stage" in lib.cfsd_last_error_string()
    rc = lib.cfsd_nn_grid_build(p, p, big, 1, None, None, 1, 4, 2, 2, 2, None)  # group stage without the sort
    assert rc == -1 and b"sorted" in lib.cfsd_last_error_string()

    def query(batch, bq, br, n=4, pp=4, cells=(2, 2, 2), nbytes=big, q=p):
        return lib.cfsd_nn_points_grid(q, p, nbytes, None, p, p, None, batch, bq, br, n, pp, *cells, None)

    assert query(1, 1, 1, q=None) == -1 and b"null" in lib.cfsd_last_error_string()
    assert query(1, 1, 1, n=0) == -1 and b"bad sizes" in lib.cfsd_last_error_string()
    assert query(4, 2, 1) == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()  # batch 2 against 4
    assert query(4, 4, 3) == -1 and b"must each be 1 or 4" in lib.cfsd_last_error_string()
    assert query(1, 1, 1, cells=(2, 2, 200)) == -1 and b"outside 1..128" in lib.cfsd_last_error_string()
    assert query(1, 1, 1, nbytes=ctypes.c_size_t(16)) == -2 and b"grid buffer" in lib.cfsd_last_error_string()


@pytest.mark.parametrize("cells", [(0, 4, 4), (4, 4, 129), (4, -1, 4), (4, 4), (4, 4, 4, 4), (2.0, 2, 2), "444", 8,
                                   (True, 2, 2)])
def test_point_grid_rejects_bad_cells(cells):
    with pytest.raises(ValueError, match="cells="):
        ops.PointGrid(torch.zeros(1, 10, 3), cells=cells)


def test_host_tensors_never_reach_a_kernel():
    with pytest.raises(ValueError, match="device"):
        ops.PointGrid(torch.zeros(1, 10, 3), cells=(2, 2, 2))
    with pytest.raises(ValueError, match="device"):
        ops.PointGrid(torch.zeros(10, 3))
    with pytest.raises(ValueError, match="PointGrid"):
        ops.nn_points_grid(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def test_bad_search_raises():
    x, y = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    for bad in ("tree", "auto", None, 1, "Grid"):
        with pytest.raises(ValueError, match="search="):
            ops.chamfer_distance(x, y, search=bad)
        with pytest.raises(ValueError, match="search="):
            fitting.fit_points(lambda z: z, torch.zeros(9, 3), torch.zeros(2, 3), [0, 4], None, None, torch.zeros(3),
                               search=bad)
    with pytest.raises(ValueError, match="surface"):  # the surface term keeps its own search
        faces = torch.zeros(2, 3, dtype=torch.int32)
        fitting.fit_points(lambda z: z, torch.zeros(9, 3), torch.zeros(2, 3), [0, 4], None, None, torch.zeros(3),
                           search="grid", target_faces=faces, template_faces=faces)


def _stub_grid(batch, p):
    """A PointGrid's host-side fields without a device (nothing is launched:
    the batch rule is checked before any tensor is touched)."""
    g = ops.PointGrid.__new__(ops.PointGrid)
    g.batch, g.p, g.cells, g.perm, g.queries = batch, p, (2, 2, 2), None, None
    g.points = torch.zeros(batch, p, 3)
    return g


@pytest.mark.parametrize("bq,br", [(2, 3), (4, 2), (3, 16)])
def test_mismatched_batch_sizes_raise(bq, br):
    with pytest.raises(ValueError, match="must be equal or 1"):
        ops.nn_points_grid(torch.zeros(bq, 5, 3), _stub_grid(br, 7))


def test_default_cell_rule_depends_on_point_count_only():
    seen = []
    for p in (1, 2, 15, 17, 300, 2000, 17039, 68000, 272000, 1090000, 10 ** 8):
        cells = ops.default_grid_cells(p)
        assert len(cells) == 3 and len(set(cells)) == 1
        assert all(isinstance(g, int) and 1 <= g <= ops.NN_GRID_MAX for g in cells)
        seen.append(cells[0])
    assert seen == sorted(seen) and seen[0] == 1 and seen[-1] == ops.NN_GRID_MAX  # grows with P, capped
    assert ops._grid_cells(None, 17039) == ops.default_grid_cells(17039)
    assert ops._grid_cells((3, 5, 128), 17039) == (3, 5, 128)
