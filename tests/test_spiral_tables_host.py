"""The synthetic spiral tables (``tests/golden/spiral_tables.py``) have the
properties the specialised SpiralConv tests rely on, at the sizes those tests
use: every generator asserts its own property on return, and here the
properties are restated through ``topology.inverse_spiral`` /
``topology.inverse_flat`` -- the tables the kernels actually read.  CPU only."""
import numpy as np
import pytest

import cfsd_loader

cfsd_loader.load()
import spiral_tables as T  # noqa: E402
from craniofacialsd_vae_amd import topology  # noqa: E402

# (rows, vsrc): decoder form, Enblock form, three rows per source vertex
GEOMS = [(2731, 2731), (683, 2731), (2733, 911), (5500, 22001)]


def list_lengths(table, vsrc):
    ptr, rows, head = topology.inverse_spiral(table, vsrc)
    n = np.diff(ptr).reshape(vsrc, T.SEQ)
    # the inline head holds min(n, INV_HEAD) rows of every list
    assert np.array_equal((head >= 0).sum(1).reshape(vsrc, T.SEQ), np.minimum(n, topology.INV_HEAD))
    return n


def test_inv_head_constant():
    assert T.INV_HEAD == topology.INV_HEAD and T.SEQ == 9


@pytest.mark.parametrize("rows,vsrc", GEOMS + [(37, 37)])
def test_random_repeats_vertices(rows, vsrc):
    t = T.random(rows, vsrc, seed=3)
    assert any(len(set(r)) < T.SEQ for r in t)
    assert np.array_equal(t, T.random(rows, vsrc, seed=3))  # deterministic
    assert not np.array_equal(t, T.random(rows, vsrc, seed=4))


@pytest.mark.parametrize("rows,vsrc", GEOMS)
def test_hubs_long_lists_beside_short_ones(rows, vsrc):
    t = T.hubs(rows, vsrc, seed=1)
    n = list_lengths(t, vsrc)
    assert n.max() > 8 * topology.INV_HEAD
    # an aligned group of 16 vertices whose lists of one slot include 0, 1 and more than the head
    found = 0
    for u0 in range(0, vsrc - 15, 16):
        grp = n[u0:u0 + 16]
        found += int((((grp == 0).any(0)) & ((grp == 1).any(0)) & ((grp > topology.INV_HEAD).any(0))).any())
    assert found >= 5
    # about half of all entries sit on five vertices
    assert np.sort(T.fan_in(t, vsrc))[-5:].sum() >= 0.4 * t.size


@pytest.mark.parametrize("rows,vsrc", GEOMS + [(37, 37), (37, 149)])
def test_head_edge_lists_on_both_sides_of_the_head(rows, vsrc):
    t = T.head_edge(rows, vsrc, seed=2)
    n = list_lengths(t, vsrc)
    keys = T.head_edge_keys(vsrc)
    assert sorted({k[2] for k in keys}) == [3, 4, 5, 6] and 3 < topology.INV_HEAD + 1 < 6
    for u, s, want in keys:
        assert n[u, s] == want
    first, mid, last = keys[:4], keys[4:8], keys[8:]
    assert all(u < 16 for u, _, _ in first) and all(u >= vsrc - 5 for u, _, _ in last)
    assert all(16 <= u < vsrc - 5 for u, _, _ in mid)  # neither of the two
    # gaps: the first and last vertex, and from GAP_RUN_MIN vertices on two whole 32-row tiles
    f = T.fan_in(t, vsrc)
    assert f[0] == 0 and f[vsrc - 1] == 0
    if vsrc >= T.GAP_RUN_MIN:
        start = (vsrc // 4) // 32 * 32
        assert start % 32 == 0 and not f[start:start + 64].any()
    else:
        assert len(T.gap_vertices(vsrc)) == 2


def test_head_edge_without_gaps_uses_every_other_vertex():
    t = T.head_edge(2731, 2731, seed=2, gaps=False)
    assert T.fan_in(t, 2731)[[0, 2730]].all()


@pytest.mark.parametrize("rows,vsrc", GEOMS + [(37, 37)])
def test_one_vertex_rows(rows, vsrc):
    t = T.one_vertex_rows(rows, vsrc, seed=5)
    same = [r for r in t if len(set(r)) == 1]
    assert len(same) >= (rows + 6) // 7
    n = list_lengths(t, vsrc)
    assert (n[same[0][0]] >= 1).all()  # that vertex has a row on each of its nine keys


@pytest.mark.parametrize("rows,vsrc", [(37, 149), (911, 3644), (5500, 22001)])
@pytest.mark.parametrize("fan", [4, 8, 12, 16, 17])
def test_fan_tables_give_every_flat_width(fan, rows, vsrc):
    t = T.fan_table(rows, vsrc, fan, seed=fan)
    assert T.fan_in(t, vsrc).max() == fan
    flat, width = topology.inverse_flat(t, vsrc)
    if fan == 17:
        assert flat is None and width == 0
        return
    assert width == fan and flat.shape == (vsrc, fan)
    # ascending positions first, then -1 padding; every padding of the last int4 group occurs
    n = (flat >= 0).sum(1)
    assert np.array_equal(n, T.fan_in(t, vsrc))
    assert {fan, fan - 1, fan - 2, fan - 3} <= set(n.tolist())
    assert n[0] == 0 and n[vsrc - 1] == 0
