"""Deferred weight gradients, one case per slab layout and producer.

Every conv entry point that can leave its weight-gradient partial sums
("slabs") in the workspace is run twice on the same operands: once reducing
at once (dw / db given), once deferred (dw = db = None) with the slabs summed
later by ``dw_reduce_batch``.  Both reduces take the slab layout from one
derivation in the library (``slab_set`` in spiral_conv.hip, keyed by the
``CFSD_DW_*`` code the deferred descriptor carries), so the two results are
the same sums in the same order: ``torch.equal``.  The always-deferred bf16
pair launches are compared with the immediate ``spiral_conv_bwd_weight_x`` on
the same operands, whose slabs they share.  Accuracy against float64 is
checked by test_gpu_parity.py / test_gpu_vm32.py / test_gpu_bf16.py.

The index tables are synthetic, ``idx[r, s] = (r * stride + OFFS[s]) % vsrc``:
full rows (stride 1, rows = vsrc) give every source vertex fan-in 9 (flat
width 12), stride 4 with rows = vsrc / 4 a row subset (an Enblock conv).
The shapes are the smallest at which each layout branch is taken: few-row
unit slabs below 65536 = batch x rows (batch 4 x 50 rows: 7 row chunks, not a
whole number of 4-chunk groups), persistent unit slabs from there (16 x 4100),
plain slabs of the xyz input / output layers, the bf16 kernels' plain slabs.
Workspaces are exactly the queried size and start as NaN, so a slab that is
read without having been written fails the comparison.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cfsd_loader

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFFS = (0, 1, 2, 3, 5, 8, 13, 21, 34)
PLAIN, FUSED, BF16, VM32 = 0, 1, 2, 3
F32, B16 = torch.float32, torch.bfloat16

FULL_200 = (200, 200, 1)
FULL_600 = (600, 600, 1)
FULL_4100 = (4100, 4100, 1)
SUB_200 = (200, 50, 4)


def case(name, code, via, table, bsz, cin, cout, x=(F32, False), dpre=(F32, False)):
    """x / dpre: (dtype, vertex-major)."""
    return SimpleNamespace(name=name, code=code, via=via, table=table, bsz=bsz, cin=cin, cout=cout, x=x, dpre=dpre)


CASES = [
    # ---- few-row unit slabs (batch x rows < 65536)
    case("lat-32-32-weight", PLAIN, "weight", FULL_200, 16, 32, 32),
    case("lat-64-32-weight", PLAIN, "weight", FULL_200, 16, 64, 32),
    case("lat-32-64-weight", PLAIN, "weight", FULL_200, 16, 32, 64),
    case("lat-64-64-weight", PLAIN, "weight", FULL_200, 16, 64, 64),
    case("lat-32-32-weight-7-chunks", PLAIN, "weight", SUB_200, 4, 32, 32),
    case("lat-32-32-bwd-coarse-pair", FUSED, "bwd", FULL_200, 16, 32, 32),      # batch x vsrc < 8192: slot-group dx
    case("lat-64-64-bwd-coarse-pair", FUSED, "bwd", FULL_200, 16, 64, 64),
    case("lat-32-64-bwd-coarse-pair", FUSED, "bwd", FULL_200, 16, 32, 64),
    case("lat-32-32-bwd-pair", FUSED, "bwd", FULL_600, 16, 32, 32),             # 9600 source rows: list dx + dW
    case("lat-64-32-bwd-pair", FUSED, "bwd", FULL_600, 16, 64, 32),
    case("lat-32-32-rowsub", FUSED, "rowsub", SUB_200, 16, 32, 32),
    case("lat-32-64-rowsub-7-chunks", FUSED, "rowsub", SUB_200, 4, 32, 64),
    case("lat-32-32-rowsub-vm-x", FUSED, "rowsub", SUB_200, 16, 32, 32, x=(F32, True)),
    case("lat-32-32-weight_x-vm-x", PLAIN, "weight_x", FULL_200, 16, 32, 32, x=(F32, True)),
    case("lat-32-32-weight_x-vm-both", VM32, "weight_x", FULL_200, 16, 32, 32, x=(F32, True), dpre=(F32, True)),
    # ---- persistent unit slabs (batch x rows >= 65536)
    case("mfma-32-32-weight", PLAIN, "weight", FULL_4100, 16, 32, 32),
    case("mfma-32-32-weight_x-vm-both", VM32, "weight_x", FULL_4100, 16, 32, 32, x=(F32, True), dpre=(F32, True)),
    case("mfma-32-32-flat_pair", VM32, "flat_pair", FULL_4100, 16, 32, 32, x=(F32, True), dpre=(F32, True)),
    case("mfma-32-32-weight_x-vm-x", PLAIN, "weight_x", FULL_4100, 16, 32, 32, x=(F32, True)),
    # ---- plain slabs
    case("xyz-3-32-weight_x", PLAIN, "weight_x", FULL_200, 16, 3, 32),
    case("xyz-3-32-weight_x-bf16-dpre", PLAIN, "weight_x", FULL_200, 16, 3, 32, dpre=(B16, False)),
    case("xyz-3-16-weight", PLAIN, "weight", FULL_200, 16, 3, 16),
    # 32 -> 3 twice with the same sizes: only the code tells the two layouts apart
    case("out-32-3-weight", PLAIN, "weight", FULL_200, 16, 32, 3),
    case("out-32-3-bwd", FUSED, "bwd", FULL_200, 16, 32, 3),
    case("out-32-3-bwd_x", FUSED, "bwd_x", FULL_200, 16, 32, 3, x=(B16, True), dpre=(F32, True)),
    case("out-32-3-out_flat", FUSED, "out_flat", FULL_200, 16, 32, 3, x=(F32, True), dpre=(F32, True)),
    # ---- the bf16 kernels' plain slabs
    case("bf16-32-32-weight_x-vm", BF16, "weight_x", FULL_200, 16, 32, 32, x=(B16, True), dpre=(B16, True)),
    case("bf16-64-32-weight_x", BF16, "weight_x", FULL_200, 16, 64, 32, x=(B16, False), dpre=(B16, False)),
    case("bf16-32-32-flat_pair_bf16", BF16, "flat_pair_bf16", FULL_200, 16, 32, 32, x=(B16, True), dpre=(B16, True)),
    case("bf16-32-32-rowsub_pair_bf16", BF16, "rowsub_pair_bf16", SUB_200, 16, 32, 32, x=(B16, True)),
]


@pytest.fixture(scope="module")
def mods():
    cfsd_loader.load()
    from craniofacialsd_vae_amd import _abi, ops, topology
    return _abi, ops, topology


def make_table(topology, vsrc, rows, stride):
    idx = (np.arange(rows)[:, None] * stride + np.asarray(OFFS)[None, :]) % vsrc
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    flat, width = topology.inverse_flat(idx, vsrc)
    assert width == (12 if stride == 1 else 4)
    return SimpleNamespace(idx=dev(idx.astype(np.int32)), inv=tuple(dev(a) for a in topology.inverse_spiral(idx, vsrc)),
                           flat=(dev(flat), width))


def operand(ops, gen, shape, dtype_vm):
    dtype, vm = dtype_vm
    t = torch.randn(*shape, generator=gen).to(DEV).to(dtype)
    return ops.to_vm(t) if vm else t


def workspace_bytes(ops, c, x):
    vsrc, rows, _ = c.table
    if c.via == "weight":
        return ops.spiral_conv_bwd_weight_workspace(c.bsz, rows, 9, c.cin, c.cout)
    if c.via == "weight_x":
        return ops.spiral_conv_bwd_weight_x_workspace(c.bsz, rows, 9, c.cin, c.cout, x.dtype)
    if c.via in ("bwd", "bwd_x", "out_flat"):
        return ops.spiral_conv_bwd_workspace(c.bsz, vsrc, rows, 9, c.cin, c.cout)
    if c.via == "rowsub":
        return ops.spiral_conv_bwd_rowsub_workspace(c.bsz, vsrc, rows, 9, c.cin, c.cout)
    if c.via == "flat_pair":
        return ops.spiral_conv_bwd_flat_pair_workspace(c.bsz, rows, 9, c.cin, c.cout)
    return ops.spiral_conv_bwd_weight_x_workspace(c.bsz, rows, 9, c.cin, c.cout)  # the *_pair_bf16 launches


def produce(ops, c, T, x, dpre, w, dw, db, ws):
    """One call of the case's entry point; the DeferredDw it returns when dw is None, else None."""
    dx = torch.empty_like(x)  # (x's layout: empty_like keeps a vertex-major view's strides)
    if c.via == "weight":
        return ops.spiral_conv_bwd_weight(x, T.idx, dpre, dw, db, ws)
    if c.via == "weight_x":
        return ops.spiral_conv_bwd_weight_x(x, T.idx, dpre, dw, db, ws)
    if c.via == "flat_pair":
        return ops.spiral_conv_bwd_flat_pair(x, T.idx, dpre, T.flat, w, dw, db, dx, workspace=ws)
    if c.via == "flat_pair_bf16":
        return ops.spiral_conv_bwd_flat_pair_bf16(x, T.idx, dpre, T.flat, w.to(B16), dx, workspace=ws)
    if c.via == "rowsub_pair_bf16":
        return ops.spiral_conv_bwd_rowsub_pair_bf16(x, T.idx, dpre, T.flat, w, dx, workspace=ws)
    if c.via == "bwd":
        out = ops.spiral_conv_bwd(x, T.idx, dpre, T.inv, w, dw, db, dx=dx, workspace=ws)
    elif c.via == "bwd_x":
        out = ops.spiral_conv_bwd_x(x, T.idx, dpre, T.inv, w, dw, db, dx=dx, workspace=ws)
    elif c.via == "out_flat":
        out = ops.spiral_conv_bwd_out_flat(x, T.idx, dpre, T.flat, w, dw, db, dx=dx, workspace=ws)
    else:
        out = ops.spiral_conv_bwd_rowsub(x, T.idx, dpre, T.flat, w, dw, db, dx, workspace=ws)
    return out[1] if dw is None else None


@pytest.fixture(scope="module")
def runs(mods):
    """Every case run once: the immediate dw / db, and the deferred descriptor with its (live) workspace."""
    _, ops, topology = mods
    tables, out = {}, {}
    for i, c in enumerate(CASES):
        if c.table not in tables:
            tables[c.table] = make_table(topology, *c.table)
        T, (vsrc, rows, _) = tables[c.table], c.table
        gen = torch.Generator().manual_seed(100 + i)
        x = operand(ops, gen, (c.bsz, vsrc, c.cin), c.x)
        dpre = operand(ops, gen, (c.bsz, rows, c.cout), c.dpre)
        w = (torch.randn(c.cout, 9 * c.cin, generator=gen) * 0.1).to(DEV)
        n_ws = workspace_bytes(ops, c, x) // 4
        assert n_ws > 0, c.name
        new_ws = lambda: torch.full((n_ws,), float("nan"), device=DEV)
        dw, db = torch.full((c.cout, 9 * c.cin), float("nan"), device=DEV), torch.full((c.cout,), float("nan"), device=DEV)
        if c.via.endswith("_pair_bf16"):  # always deferred: the immediate weight_x on the same operands
            assert ops.spiral_conv_bwd_weight_x(x, T.idx, dpre, dw, db, new_ws()) is None
        else:
            assert produce(ops, c, T, x, dpre, w, dw, db, new_ws()) is None
        d = produce(ops, c, T, x, dpre, w, None, None, new_ws())
        out[c.name] = SimpleNamespace(dw=dw, db=db, d=d)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_deferred_equals_immediate(mods, runs, c):
    """The descriptor carries the expected code, and a one-item batched reduce
    of its slabs gives the immediate call's dw / db bit for bit."""
    _, ops, _ = mods
    r = runs[c.name]
    vsrc, rows, _ = c.table
    assert r.d.sizes == (c.bsz, vsrc, rows, c.cin, c.cout, c.code)
    assert torch.isfinite(r.dw).all() and torch.isfinite(r.db).all()
    dw, db = torch.full_like(r.dw, float("nan")), torch.full_like(r.db, float("nan"))
    ops.dw_reduce_batch([(r.d, dw, db)])
    assert torch.equal(dw, r.dw) and torch.equal(db, r.db)


def test_batched_reduce_of_mixed_kinds(mods, runs):
    """All deferred items through launches of at most CFSD_DW_REDUCE_MAX items,
    unit, plain, fused-small and bf16 slab sets mixed in each launch."""
    abi, ops, _ = mods
    cap = abi.CONSTANTS["CFSD_DW_REDUCE_MAX"]
    n_launch = -(-len(CASES) // cap)
    for k in range(n_launch):
        group = CASES[k::n_launch]  # strided: every launch holds cases of every section of the table
        assert 1 < len(group) <= cap and len({c.code for c in group}) == 4
        outs = [(torch.full_like(runs[c.name].dw, float("nan")), torch.full_like(runs[c.name].db, float("nan")))
                for c in group]
        ops.dw_reduce_batch([(runs[c.name].d, dw, db) for c, (dw, db) in zip(group, outs)])
        for c, (dw, db) in zip(group, outs):
            assert torch.equal(dw, runs[c.name].dw) and torch.equal(db, runs[c.name].db), c.name
