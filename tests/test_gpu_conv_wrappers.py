"""The SpiralConv wrappers of ``ops`` refuse a bad operand on the host.

Device tensors are needed (the wrappers take nothing else), but every case
raises ``ValueError`` before any launch.  Shapes as
``test_host_logic._conv_rejections``: batch 16, vsrc = rows = 40, spiral
length 9, 32 -> 32 channels (32 -> 3 for the two xyz output wrappers; 4096
vertices for the vertex-major pair, which serves nothing smaller)."""
import types

import pytest
import torch

import cfsd_loader

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import ops  # noqa: E402
from craniofacialsd_vae_amd.topology import INV_HEAD  # noqa: E402

B, V, S, C = 16, 40, 9, 32  # V: vsrc = rows
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


def _bm(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _vm(b, v, c, dtype=F32):
    return ops.vm_empty(b, v, c, dtype=dtype, device="cuda")


def _operands(src=(F32, False), dpre=(F32, False), cout=C, w_dtype=F32, nv=V, ws_floats=1 << 20):
    """A valid operand set: ``src`` = (dtype, vertex-major) of x / dx / elu_y,
    ``dpre`` the same of dpre / y; ``nv`` = vsrc = rows."""
    def act(n, c, spec):
        return _vm(B, n, c, spec[0]) if spec[1] else _bm(B, n, c, dtype=spec[0])
    return types.SimpleNamespace(
        x=act(nv, C, src), dx=act(nv, C, src), elu_y=act(nv, C, src), dpre=act(nv, cout, dpre),
        y=act(nv, cout, dpre), idx=_bm(nv, S, dtype=I32), w=_bm(cout, S * C, dtype=w_dtype),
        w16=_bm(cout, S * C, dtype=BF16), bias=_bm(cout), dw=_bm(cout, S * C), db=_bm(cout),
        inv=(_bm(nv * S + 1, dtype=I32), _bm(nv * S, dtype=I32), _bm(nv * S, INV_HEAD, dtype=I32)),
        flat=(_bm(nv, 8, dtype=I32), 8), ws=_bm(ws_floats), cout=cout, nv=nv)


# wrapper -> (operand set, call).  Every call passes every optional operand, so a case can spoil any of them.
WRAPPERS = {
    "fwd": (dict(), lambda o: ops.spiral_conv_fwd(o.x, o.idx, o.w, o.bias, ops.ACT_ELU, out=o.y, workspace=o.ws)),
    "bwd_data": (dict(), lambda o: ops.spiral_conv_bwd_data(o.dpre, o.inv, o.w, V, elu_y=o.elu_y, out=o.dx,
                                                            workspace=o.ws)),
    "bwd_weight": (dict(), lambda o: ops.spiral_conv_bwd_weight(o.x, o.idx, o.dpre, o.dw, o.db, o.ws)),
    "bwd": (dict(), lambda o: ops.spiral_conv_bwd(o.x, o.idx, o.dpre, o.inv, o.w, o.dw, o.db, dx=o.dx, elu_y=o.elu_y,
                                                  workspace=o.ws)),
    "bwd_rowsub": (dict(), lambda o: ops.spiral_conv_bwd_rowsub(o.x, o.idx, o.dpre, o.flat, o.w, o.dw, o.db, o.dx,
                                                                elu_y=o.elu_y, workspace=o.ws)),
    "bwd_rowsub_vm": (dict(src=(F32, True)),
                      lambda o: ops.spiral_conv_bwd_rowsub(o.x, o.idx, o.dpre, o.flat, o.w, o.dw, o.db, o.dx,
                                                           elu_y=o.elu_y, workspace=o.ws)),
    "bwd_data_rowsub": (dict(src=(BF16, True)),
                        lambda o: ops.spiral_conv_bwd_data_rowsub(o.dpre, o.flat, o.w, V, elu_y=o.elu_y, out=o.dx,
                                                                  workspace=o.ws)),
    "fwd_x": (dict(src=(BF16, True), dpre=(BF16, True)),
              lambda o: ops.spiral_conv_fwd_x(o.x, o.idx, o.w, o.w16, o.bias, ops.ACT_ELU, o.y)),
    "bwd_data_x": (dict(src=(BF16, True), dpre=(BF16, True)),
                   lambda o: ops.spiral_conv_bwd_data_x(o.dpre, o.inv, o.w16, V, elu_y=o.elu_y, out=o.dx)),
    "bwd_data_flat": (dict(src=(F32, True), dpre=(F32, True)),
                      lambda o: ops.spiral_conv_bwd_data_flat(o.dpre, o.flat, o.w, V, elu_y=o.elu_y, out=o.dx)),
    "bwd_weight_x": (dict(src=(BF16, True), dpre=(BF16, True)),
                     lambda o: ops.spiral_conv_bwd_weight_x(o.x, o.idx, o.dpre, o.dw, o.db, o.ws)),
    # the pair serves batch x rows >= 65536 only (below, its workspace query says 0 and the wrapper refuses the
    # shape before it looks at the workspace): vsrc = rows = 4096, 8 MB a tensor, and a 32 MB workspace
    "bwd_flat_pair": (dict(src=(F32, True), dpre=(F32, True), nv=4096, ws_floats=1 << 23),
                      lambda o: ops.spiral_conv_bwd_flat_pair(o.x, o.idx, o.dpre, o.flat, o.w, o.dw, o.db, o.dx,
                                                              elu_y=o.elu_y, workspace=o.ws)),
    "bwd_flat_pair_bf16": (dict(src=(BF16, True), dpre=(BF16, True)),
                           lambda o: ops.spiral_conv_bwd_flat_pair_bf16(o.x, o.idx, o.dpre, o.flat, o.w16, o.dx,
                                                                        elu_y=o.elu_y, workspace=o.ws)),
    "bwd_rowsub_pair_bf16": (dict(src=(BF16, True)),
                             lambda o: ops.spiral_conv_bwd_rowsub_pair_bf16(o.x, o.idx, o.dpre, o.flat, o.w, o.dx,
                                                                            elu_y=o.elu_y, workspace=o.ws)),
    "bwd_x": (dict(src=(BF16, True), dpre=(F32, True), cout=3),
              lambda o: ops.spiral_conv_bwd_x(o.x, o.idx, o.dpre, o.inv, o.w, o.dw, o.db, dx=o.dx, elu_y=o.elu_y,
                                              workspace=o.ws)),
    "bwd_out_flat": (dict(src=(F32, True), dpre=(F32, True), cout=3),
                     lambda o: ops.spiral_conv_bwd_out_flat(o.x, o.idx, o.dpre, o.flat, o.w, o.dw, o.db, dx=o.dx,
                                                            elu_y=o.elu_y, workspace=o.ws)),
}

# defect -> (operands it replaces, given the valid set; the operand the message must name)
DEFECTS = {
    "idx int64": (lambda o: dict(idx=_bm(o.nv, S, dtype=torch.int64)), r"\bidx\b"),
    "inv_ptr int64": (lambda o: dict(inv=(_bm(o.nv * S + 1, dtype=torch.int64),) + o.inv[1:]), r"\binv_ptr\b"),
    "inv_row int64": (lambda o: dict(inv=(o.inv[0], _bm(o.nv * S, dtype=torch.int64), o.inv[2])), r"\binv_row\b"),
    "inv_head width": (lambda o: dict(inv=o.inv[:2] + (_bm(o.nv * S, INV_HEAD + 1, dtype=I32),)), r"\binv_head\b"),
    "inv_flat int64": (lambda o: dict(flat=(_bm(o.nv, 8, dtype=torch.int64), 8)), r"\binv_flat\b"),
    "inv_flat rows": (lambda o: dict(flat=(_bm(o.nv + 1, 8, dtype=I32), 8)), r"\binv_flat\b"),
    "dw without db": (lambda o: dict(db=None), r"\bdb\b"),
    "db without dw": (lambda o: dict(dw=None), r"\bdw\b"),
    "w shape": (lambda o: dict(w=_bm(o.cout, S * C + 1, dtype=o.w.dtype)), r"\bw\b"),
    "w16 shape": (lambda o: dict(w16=_bm(o.cout, S * C + 1, dtype=BF16)), r"\bw(_bf)?16\b"),
    "bias shape": (lambda o: dict(bias=_bm(o.cout + 1)), r"\bbias\b"),
    "dpre shape": (lambda o: dict(dpre=(_vm if ops.is_vm(o.dpre) else _bm)(B, o.nv + 1, o.cout, dtype=o.dpre.dtype)),
                   r"\bdpre\b"),
    "elu_y shape": (lambda o: dict(elu_y=(_vm if ops.is_vm(o.elu_y) else _bm)(B, o.nv + 1, C, dtype=o.elu_y.dtype)),
                    r"\belu_y\b"),
    "elu_y dtype": (lambda o: dict(elu_y=_vm(B, o.nv, C, dtype=F32 if o.elu_y.dtype == BF16 else BF16)), r"\belu_y\b"),
    "y shape": (lambda o: dict(y=(_vm if ops.is_vm(o.y) else _bm)(B, o.nv + 1, o.cout, dtype=o.y.dtype)), r"\b(y|out)\b"),
    "dx shape": (lambda o: dict(dx=(_vm if ops.is_vm(o.dx) else _bm)(B, o.nv, C + 1, dtype=o.dx.dtype)), r"\b(dx|out)\b"),
    "workspace too small": (lambda o: dict(ws=_bm(1)), r"\bworkspace\b"),
    "workspace missing": (lambda o: dict(ws=None), r"\bworkspace\b"),
    # the deferred bf16 slabs: one float short of what the library's own query asks for
    "bf16 slabs one float short": (
        lambda o: dict(ws=_bm(ops.spiral_conv_bwd_weight_x_workspace(B, o.nv, S, C, o.cout) // 4 - 1)),
        r"\bworkspace\b"),
    "batch-major x": (lambda o: dict(x=_bm(B, o.nv, C, dtype=o.x.dtype)), r"\bx\b"),
    "batch-major dpre": (lambda o: dict(dpre=_bm(B, o.nv, o.cout, dtype=o.dpre.dtype)), r"\bdpre\b"),
    "batch-major dx": (lambda o: dict(dx=_bm(B, o.nv, C, dtype=o.dx.dtype)), r"\bdx\b"),
    "batch-major elu_y": (lambda o: dict(elu_y=_bm(B, o.nv, C, dtype=o.elu_y.dtype)), r"\belu_y\b"),
    "vertex-major elu_y": (lambda o: dict(elu_y=_vm(B, o.nv, C, dtype=o.elu_y.dtype)), r"\belu_y\b"),
}

_IDX = ["idx int64"]
_INV = ["inv_ptr int64", "inv_head width"]
_FLAT = ["inv_flat int64", "inv_flat rows"]
_PAIR = ["dw without db", "db without dw"]
_SRC = ["elu_y shape", "dx shape"]
CASES = {
    "fwd": _IDX + ["w shape", "bias shape", "y shape", "workspace too small"],
    "bwd_data": _INV + _SRC + ["w shape", "workspace too small", "vertex-major elu_y"],
    "bwd_weight": _IDX + _PAIR + ["dpre shape", "workspace too small", "workspace missing"],
    "bwd": _IDX + _INV + _PAIR + _SRC + ["w shape", "dpre shape", "workspace too small"],
    "bwd_rowsub": _IDX + _FLAT + _PAIR + _SRC + ["w shape", "dpre shape", "workspace too small",
                                                 "vertex-major elu_y"],
    "bwd_rowsub_vm": _IDX + _FLAT + _PAIR + _SRC + ["w shape", "workspace too small", "batch-major dx",
                                                    "batch-major elu_y"],
    "bwd_data_rowsub": _FLAT + _SRC + ["w shape", "elu_y dtype", "workspace too small", "batch-major elu_y"],
    "fwd_x": _IDX + ["w shape", "w16 shape", "bias shape", "y shape"],
    "bwd_data_x": _INV + _SRC + ["w16 shape", "elu_y dtype", "batch-major elu_y"],
    "bwd_data_flat": _FLAT + _SRC + ["w shape", "elu_y dtype", "batch-major elu_y"],
    "bwd_weight_x": _IDX + _PAIR + ["dpre shape", "workspace too small", "workspace missing"],
    "bwd_flat_pair": _IDX + _FLAT + _PAIR + _SRC + ["w shape", "dpre shape", "workspace too small", "batch-major x",
                                                    "batch-major dpre", "batch-major dx", "batch-major elu_y"],
    "bwd_flat_pair_bf16": _IDX + _FLAT + _SRC + ["w16 shape", "dpre shape", "workspace missing", "batch-major x",
                                                 "batch-major dpre", "batch-major dx", "batch-major elu_y"],
    "bwd_rowsub_pair_bf16": _IDX + _FLAT + _SRC + ["w shape", "dpre shape", "workspace missing", "batch-major x",
                                                   "batch-major dx", "batch-major elu_y"],
    "bwd_x": _IDX + ["inv_head width"] + _PAIR + _SRC + ["w shape", "dpre shape", "workspace too small",
                                                        "batch-major dx", "batch-major elu_y"],
    "bwd_out_flat": _IDX + _FLAT + _PAIR + _SRC + ["w shape", "dpre shape", "workspace too small", "batch-major x",
                                                   "batch-major dpre", "batch-major dx", "batch-major elu_y"],
}

# Host checks that are NEW with the shared helpers (the wrappers used to hand these operands to the library,
# whose own check raised CfsdError): the two *_pair_bf16 wrappers compare the workspace with the size of the
# deferred bf16 slabs, and spiral_conv_bwd_x checks the whole inverse triple, not inv_head alone.
NEW_CHECKS = {
    "bwd_flat_pair_bf16": ["workspace too small", "bf16 slabs one float short"],
    "bwd_rowsub_pair_bf16": ["workspace too small", "bf16 slabs one float short"],
    "bwd_x": ["inv_ptr int64", "inv_row int64"],
}


@pytest.fixture(scope="module")
def operand_sets():
    return {name: _operands(**spec) for name, (spec, _) in WRAPPERS.items()}


def test_every_wrapper_has_cases():
    assert set(CASES) == set(WRAPPERS)
    for name, defects in CASES.items():
        assert len(defects) == len(set(defects)) >= 4, name
        assert all(d in DEFECTS for d in defects), name


@pytest.mark.parametrize("name,defect", [(n, d) for n, ds in CASES.items() for d in ds])
def test_conv_wrapper_rejects_before_launch(operand_sets, name, defect):
    _rejects(operand_sets, name, defect)


@pytest.mark.parametrize("name,defect", [(n, d) for n, ds in NEW_CHECKS.items() for d in ds])
def test_new_host_check_rejects_before_launch(operand_sets, name, defect):
    """New behaviour: ValueError on the host where the library's check used to raise CfsdError."""
    _rejects(operand_sets, name, defect)


def _rejects(operand_sets, name, defect):
    good = operand_sets[name]
    spoil, match = DEFECTS[defect]
    bad = types.SimpleNamespace(**{**vars(good), **spoil(good)})
    with ops._abi.trace_launches() as launched:
        with pytest.raises(ValueError, match=match):
            WRAPPERS[name][1](bad)
    assert launched == []
