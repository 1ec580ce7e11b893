"""The general-shape SpiralConv kernels (cfsd_spiral_conv_gen_*) against an
fp64 restatement (index_select + matmul; dx by index_add_; dW by G^T.dY).

Tolerance (derived, not measured).  The fp32 MFMA is a k-ordered fmaf chain,
so a sum of n terms in any order has |err| <= gamma_n * sum|terms| with
gamma_n = n u / (1 - n u), u = 2^-24:

    forward   n = seq * cin + 1           terms |w| |x| and |bias|
    dx        n = entries(u) * cout       terms |dpre| |w| (0 entries: exactly 0)
    dW / db   n = batch * rows            terms |dpre| |x| / |dpre|

(dx adds the dpre rows of one (vertex, slot) list before the product with the
slot's weights: a term then passes E_s - 1 additions and one fmaf per output
channel of every non-empty slot, at most entries * cout roundings in all.)
sum|terms| is computed in fp64 from absolute values.  ELU and its derivative
are 1-Lipschitz, so the sum's error passes through unamplified, and one more
fp32 rounding (u, relative) is allowed for them:

* forward: y = exp(v) - 1 rounds exp(v) <= 1 before an exact subtraction, so
  the u is taken of max(1, |y|);
* dx: the factor g = y + 1 is exact for an ELU output y = fl(e - 1) of an fp32
  e = exp(v) < 1 (e - 1 is exact for e >= 1/2, and below that y is a multiple
  of 2^-24 in [-1, -1/2), so y + 1 is one too); elu_y is built that way here,
  as the forward kernels produce it, and the u covers the product g * sum.
"""
import numpy as np
import pytest
import torch

from conv_cases import DEV, Case, check, check_case, gamma, run_kernels  # (loads libcfsd)
from craniofacialsd_vae_amd import model as M
from craniofacialsd_vae_amd import ops, topology

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (7, 3, 8), (12, 8, 20), (4, 20, 3), (5, 40, 36), (9, 48, 32)]
GEOMS = [(70, 70), (70, 37), (9, 5)]
BATCHES = (1, 3)


@pytest.mark.parametrize("vsrc,rows", GEOMS)
@pytest.mark.parametrize("seq,cin,cout", SHAPES)
def test_general_kernels_match_fp64(seq, cin, cout, vsrc, rows):
    assert not ops.spiral_conv_has_shape(ops.CONV_FWD, seq, cin, cout)  # ops routes these to the general family
    for batch in BATCHES:
        c = Case(batch, vsrc, rows, seq, cin, cout, seed=1000 * seq + 10 * cin + cout + batch)
        out, ws = run_kernels(c)
        check_case(c, out)
        # a vertex in no spiral: exactly 0, with and without the ELU factor
        assert int((c.idx == c.absent).sum()) == 0
        assert torch.count_nonzero(out["dx"][:, c.absent]) == 0
        assert torch.count_nonzero(out["dx_elu"][:, c.absent]) == 0
        # deferred dW: the slabs stay in the workspace, the reduce gives the immediate result bit for bit
        d = c.d
        ws2 = torch.empty_like(ws)
        item = ops.spiral_conv_bwd_weight(d["x"], d["idx"], d["dpre"], None, None, ws2)
        assert isinstance(item, ops.DeferredGenDw)
        dw2, db2 = torch.full_like(d["w"], 7.0), torch.full_like(d["b"], 7.0)
        ops.spiral_conv_gen_dw_reduce(item, dw2, db2)
        assert torch.equal(dw2, out["dw"]) and torch.equal(db2, out["db"])
        # ... also as an item of the batched reduce
        dw3, db3 = torch.full_like(d["w"], 7.0), torch.full_like(d["b"], 7.0)
        ops.dw_reduce_batch([(item, dw3, db3)])
        assert torch.equal(dw3, out["dw"]) and torch.equal(db3, out["db"])
        # a second call on the same inputs: bit-identical
        again, _ = run_kernels(c)
        for k in out:
            assert torch.equal(out[k], again[k]), (k, c.shape)


def test_subset_rows_and_long_lists():
    """vsrc = 9 puts many rows on every (vertex, slot) key: lists far longer
    than the inline head of the specialised kernels' inverse table."""
    c = Case(3, 9, 70, 12, 8, 20, seed=5)
    ptr = c.inv[0].cpu().numpy()
    assert np.diff(ptr).max() > 2 * topology.INV_HEAD
    out, _ = run_kernels(c)
    check_case(c, out)
    assert torch.count_nonzero(out["dx"][:, c.absent]) == 0


def test_two_column_tiles_per_wave():
    """From 2048 row tiles (65 536 rows) a wave of the forward and dx kernels takes two column
    tiles; (5, 40, 36) has a second, partial one in both (cout 36, cin 40).  The smallest size on
    that path, one tile past the threshold with a partial last row tile."""
    n = 2049 * 32 + 8
    c = Case(1, n, n, 5, 40, 36, seed=21)
    out, _ = run_kernels(c)
    check_case(c, out)
    assert torch.count_nonzero(out["dx"][:, c.absent]) == 0


def test_many_rows_one_column_tile():
    """Below 2048 row tiles the dx kernel splits a tile's spiral slots over the waves of a
    workgroup (every smaller case here); from there on a wave walks all slots of its own tile.
    (12, 8, 20) at the same size: that path with one column tile."""
    n = 2049 * 32 + 8
    c = Case(1, n, n, 12, 8, 20, seed=22)
    out, _ = run_kernels(c)
    check_case(c, out)
    assert torch.count_nonzero(out["dx"][:, c.absent]) == 0


def test_forced_general_agrees_with_specialised():
    """(9, 32, 32) at 70 rows has specialised instances: both families are
    within the same bound of the fp64 restatement (no bit-equality asked:
    their summation orders differ)."""
    for batch in BATCHES:
        c = Case(batch, 70, 70, 9, 32, 32, seed=77 + batch)
        assert all(ops.spiral_conv_has_shape(r, 9, 32, 32) for r in range(3))
        spec, _ = run_kernels(c)
        gen, _ = run_kernels(c, general=True)
        check_case(c, spec)
        check_case(c, gen)
        assert torch.count_nonzero(gen["dx"][:, c.absent]) == 0


def test_spiral_conv_module_autograd():
    """model.SpiralConv(8, 20, indices[70, 12]) forward and backward through
    autograd against the restatement (refused before the general kernels)."""
    c = Case(3, 70, 70, 12, 8, 20, seed=11)
    conv = M.SpiralConv(8, 20, c.idx.to(DEV)).to(DEV)
    assert repr(conv) == "SpiralConv(8, 20, seq_length=12)"
    with torch.no_grad():
        conv.layer.weight.copy_(c.d["w"])
        conv.layer.bias.copy_(c.d["b"])
    x = c.d["x"].clone().requires_grad_(True)
    y = conv(x)
    check("module fwd", y.detach(), c.pre, gamma(c.n_fwd) * c.pre_abs, c.shape)
    y.backward(c.d["dpre"])
    check("module dx", x.grad, c.dx, gamma(c.n_dx) * c.dx_abs, c.shape)
    check("module dw", conv.layer.weight.grad, c.dw, gamma(c.n_dw) * c.dw_abs, c.shape)
    check("module db", conv.layer.bias.grad, c.db, gamma(c.n_dw) * c.db_abs, c.shape)


@pytest.mark.parametrize("cin,cout", [(32, 1), (32, 2), (64, 1), (64, 2), (32, 3), (64, 32)])
@pytest.mark.parametrize("with_dx", [False, True])
def test_fused_backward_stays_specialised(monkeypatch, cin, cout, with_dx):
    """``ops.spiral_conv_bwd`` of a shape ``cfsd_spiral_conv_bwd`` takes is that one library call
    and no general kernel: the small-output layers 32 / 64 -> 1, 2 have no separate dx / dW
    instance, yet the fused launch has them.  A shape it refuses is two general calls."""
    c = Case(2, 70, 70, 9, cin, cout, seed=200 + cin + cout)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    dw, db = torch.empty(cout, 9 * cin, device=DEV), torch.empty(cout, device=DEV)
    dx = torch.empty(2, 70, cin, device=DEV) if with_dx else None
    ops.spiral_conv_bwd(c.d["x"], c.d["idx"], c.d["dpre"], c.inv, c.d["w"], dw, db, dx=dx)
    assert names == ["cfsd_spiral_conv_bwd"], names
    check("fused dw", dw, c.dw, gamma(c.n_dw) * c.dw_abs, c.shape)
    check("fused db", db, c.db, gamma(c.n_dw) * c.db_abs, c.shape)
    if with_dx:
        check("fused dx", dx, c.dx, gamma(c.n_dx) * c.dx_abs, c.shape)
    if (cin, cout) == (32, 1):  # and a shape the library refuses, through the same function
        g = Case(2, 70, 70, 9, 48, 32, seed=7)
        del names[:]
        dw, db = torch.empty(32, 9 * 48, device=DEV), torch.empty(32, device=DEV)
        ops.spiral_conv_bwd(g.d["x"], g.d["idx"], g.d["dpre"], g.inv, g.d["w"], dw, db,
                            dx=torch.empty_like(g.d["x"]) if with_dx else None)
        assert names == (["cfsd_spiral_conv_gen_bwd_data"] if with_dx else []) + ["cfsd_spiral_conv_gen_bwd_weight"]
