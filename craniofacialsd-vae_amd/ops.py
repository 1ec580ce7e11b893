"""Typed host wrappers over the libcfsd C ABI.

Every wrapper validates shapes/dtypes/devices on the host BEFORE launching
(an out-of-range launch on the GPU would fault the device), then launches on
the current torch stream with no synchronisation.  Outputs may be passed in
(pre-allocated, graph-capture friendly) or are allocated with ``torch.empty``.
"""
import ctypes

import torch

from . import _abi
from ._abi import call, ptr, stream_ptr
from .topology import INV_HEAD

_H = _abi.CONSTANTS  # the integer CFSD_* #defines of include/cfsd.h, by name
ACT_NONE, ACT_ELU = _H["CFSD_ACT_NONE"], _H["CFSD_ACT_ELU"]
DT_F32, DT_BF16 = _H["CFSD_DT_F32"], _H["CFSD_DT_BF16"]
_DTYPES = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}


def _need(t, shape, dtype=torch.float32, name="tensor"):
    if t is None:
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _dt(t, name="tensor"):
    if t.dtype not in _DTYPES:
        raise ValueError(f"{name}: dtype {t.dtype}, expected float32 or bfloat16")
    return _DTYPES[t.dtype]


def _needx(t, shape, name="tensor"):
    """_need for a mixed-precision operand (fp32 or bf16)."""
    if t is None:
        raise ValueError(f"{name} is required")
    return _need(t, shape, t.dtype if t.dtype in _DTYPES else torch.float32, name)


# ------------------------------------------------------------------ layouts
VM = _H["CFSD_VM"]  # vertex-major storage flag of a *_dt argument


def is_vm(t):
    """True for a logical [B, V, C] view of a VERTEX-MAJOR [V, B, C] buffer
    (``vm_empty`` / ``to_vm``): element (b, v, c) at (v*B + b)*C + c, the
    rows of one vertex in every mesh of the batch contiguous."""
    if t is None or t.dim() != 3 or t.is_contiguous():
        return False
    b, v, c = t.shape
    return t.stride() == (c, b * c, 1)


def vm_empty(bsz, nv, c, dtype=torch.float32, device="cuda"):
    """Uninitialised vertex-major tensor, seen as [bsz, nv, c]."""
    return torch.empty((nv, bsz, c), dtype=dtype, device=device).permute(1, 0, 2)


def to_vm(t):
    """Vertex-major copy of a [B, V, C] tensor (same logical values)."""
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def _needl(t, shape, name="tensor", dtype=None):
    """A mixed-precision [B, V, C] operand in either layout: batch-major
    (contiguous) or vertex-major (``is_vm``)."""
    if t is None:
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    want = dtype if dtype is not None else (t.dtype if t.dtype in _DTYPES else torch.float32)
    if t.dtype != want:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {want}")
    if not (t.is_contiguous() or is_vm(t)):
        raise ValueError(f"{name} must be contiguous (batch-major) or a vertex-major view")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _st(t, name="tensor"):
    """Storage descriptor of a mixed-precision operand: type | CFSD_VM."""
    return _dt(t, name) | (VM if is_vm(t) else 0)


def _same_layout(a, b, what):
    if a is not None and b is not None and is_vm(a) != is_vm(b):
        raise ValueError(f"{what} must share one layout")


def _out(out, shape, like, name="out"):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    return _need(out, shape, name=name)


# ------------------------------------------------------------------ spiral conv
# roles of spiral_conv_has_shape
CONV_FWD, CONV_BWD_DATA = _H["CFSD_CONV_FWD"], _H["CFSD_CONV_BWD_DATA"]
CONV_BWD_WEIGHT, CONV_BWD_FUSED = _H["CFSD_CONV_BWD_WEIGHT"], _H["CFSD_CONV_BWD_FUSED"]
GEN_MAX_SEQ, GEN_MAX_CH = _H["CFSD_GEN_MAX_SEQ"], _H["CFSD_GEN_MAX_CH"]
# which launch left a deferred weight gradient's slabs (cfsd_dw_slabs.fused)
DW_PLAIN, DW_FUSED = _H["CFSD_DW_PLAIN"], _H["CFSD_DW_FUSED"]
DW_BF16, DW_VM32 = _H["CFSD_DW_BF16"], _H["CFSD_DW_VM32"]


def spiral_conv_has_shape(role, seq, cin, cout):
    """True when the specialised fp32 batch-major kernels of ``role`` (CONV_FWD,
    CONV_BWD_DATA, CONV_BWD_WEIGHT) have an instance for this shape; any other
    shape inside the limits takes the general-shape entry points
    (``cfsd_spiral_conv_gen_*``).  CONV_BWD_FUSED: a small-output layer
    (32 / 64 -> 1, 2, 3) whose dx + dW ``cfsd_spiral_conv_bwd`` / ``_bwd_x``
    run as one fused launch."""
    return bool(_abi.lib().cfsd_spiral_conv_has_shape(int(role), int(seq), int(cin), int(cout)))


def spiral_conv_bwd_is_general(seq, cin, cout, dx=True):
    """True when ``cfsd_spiral_conv_bwd`` refuses the shape, so the backward
    (dW, and dx unless ``dx`` is False: the first Enblock) is two launches with
    the general kernels wherever a product has no instance.  The library takes
    the fused small-output layers, and any shape its dW and (with dx) its dx
    entry points both have."""
    if spiral_conv_has_shape(CONV_BWD_FUSED, seq, cin, cout):
        return False
    roles = (CONV_BWD_WEIGHT,) + ((CONV_BWD_DATA,) if dx else ())
    return not all(spiral_conv_has_shape(r, seq, cin, cout) for r in roles)


def spiral_conv_vm_has_shape(seq, cin, cout):
    """True when the vertex-major / mixed-precision entry points (``_fwd_x``,
    ``_bwd_weight_x``, ``_bwd_x``) have instances for a layer of this shape:
    the MFMA shapes, the xyz input conv, the fused small-output layers.  The
    general kernels are batch-major fp32 only, so nothing else can run
    vertex-major or in bf16."""
    return (spiral_conv_has_shape(CONV_BWD_WEIGHT, seq, cin, cout)
            or spiral_conv_has_shape(CONV_BWD_FUSED, seq, cin, cout))


def _check_gen_limits(seq, cin, cout):
    if not (1 <= seq <= GEN_MAX_SEQ and 1 <= cin <= GEN_MAX_CH and 1 <= cout <= GEN_MAX_CH):
        raise ValueError(f"SpiralConv of spiral length {seq}, {cin} -> {cout} channels is outside the "
                         f"general kernels' limits (length <= {GEN_MAX_SEQ}, channels <= {GEN_MAX_CH})")


def spiral_conv_workspace(bsz, vsrc, rows, seq, cin, cout):
    """Workspace of the specialised forward / dx kernels (0 for a shape without one)."""
    return int(_abi.lib().cfsd_spiral_conv_workspace(bsz, vsrc, rows, seq, cin, cout))


def _conv_ws(workspace, device, need):
    if workspace is None:
        workspace = torch.empty(need // 4 + 1, dtype=torch.float32, device=device)
    _need(workspace, None, name="workspace")
    nbytes = workspace.numel() * workspace.element_size()
    if nbytes < need:
        raise ValueError(f"conv workspace {nbytes} < {need} bytes")
    return workspace, nbytes


def _conv_dims(x, idx):
    """(bsz, vsrc, rows, seq, cin) of x [bsz, vsrc, cin] gathered through idx [rows, seq] (checked)."""
    bsz, vsrc, cin = x.shape
    rows, seq = idx.shape
    _need(idx, (rows, seq), torch.int32, "idx")
    return bsz, vsrc, rows, seq, cin


def _need_dw_db(dw, db, cout, k):
    """The dw [cout, k] / db [cout] pair: both, or neither (the reduction is deferred)."""
    if dw is not None or db is not None:
        _need(dw, (cout, k), name="dw")
        _need(db, (cout,), name="db")


def _need_inv(inv, vsrc, rows, seq):
    """The (inv_ptr, inv_row, inv_head) triple of ``topology.inverse_spiral``."""
    inv_ptr, inv_row, inv_head = inv
    _need(inv_ptr, (vsrc * seq + 1,), torch.int32, "inv_ptr")
    _need(inv_row, (rows * seq,), torch.int32, "inv_row")
    _need(inv_head, (vsrc * seq, INV_HEAD), torch.int32, "inv_head")
    return inv_ptr, inv_row, inv_head


def _need_flat(flat, vsrc):
    """The (table, width) pair of ``topology.inverse_flat``."""
    table, width = flat
    _need(table, (vsrc, width), torch.int32, "inv_flat")
    return table, width


def _need_like(ref, ref_name, shape, dtype, **operands):
    """Optional operands (dx, elu_y) of ``shape`` and ``dtype`` that share ``ref``'s layout."""
    for name, t in operands.items():
        if t is not None:
            _needl(t, shape, name, dtype)
            _same_layout(ref, t, f"{ref_name} and {name}")


def _need_vm(t, shape, name, dtype):
    if not is_vm(_needl(t, shape, name, dtype)):
        raise ValueError(f"{name} must be vertex-major")


def spiral_conv_fwd(x, idx, w, b, act=ACT_NONE, out=None, workspace=None, general=False):
    """y[b, r] = act(b + W . concat_s x[b, idx[r, s]])  (model.py:27-41).
    A shape without a specialised instance takes the general-shape kernel;
    ``general=True`` forces it (tests, tools/bench_general_conv.py)."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), w.shape[0]
    _need(x, None, name="x")
    _need(w, (cout, seq * cin), name="w")
    if b is not None:
        _need(b, (cout,), name="bias")
    y = _out(out, (bsz, rows, cout), x)
    if general or not spiral_conv_has_shape(CONV_FWD, seq, cin, cout):  # no instance: the general kernel
        _check_gen_limits(seq, cin, cout)
        call("cfsd_spiral_conv_gen_fwd", ptr(x), ptr(idx), ptr(w), ptr(b), ptr(y), bsz, vsrc, rows, seq, cin, cout,
             act, stream_ptr())
        return y
    ws, nb = _conv_ws(workspace, x.device, spiral_conv_workspace(bsz, vsrc, rows, seq, cin, cout))
    call("cfsd_spiral_conv_fwd", ptr(x), ptr(idx), ptr(w), ptr(b), ptr(y), ptr(ws),
         ctypes.c_size_t(nb), bsz, vsrc, rows, seq, cin, cout, act, stream_ptr())
    return y


def spiral_conv_bwd_data(dpre, inv, w, vsrc, elu_y=None, out=None, workspace=None, general=False):
    """dx[b, u] = g * sum_{(r,s) in inv(u)} W_s^T dpre[b, r]; ``inv`` is the
    (inv_ptr, inv_row, inv_head) triple of ``topology.inverse_spiral``.
    ``general``: as :func:`spiral_conv_fwd`."""
    bsz, rows, cout = dpre.shape
    seq = (inv[0].numel() - 1) // vsrc
    cin = w.shape[1] // seq
    _need(dpre, None, name="dpre")
    inv_ptr, inv_row, inv_head = _need_inv(inv, vsrc, rows, seq)
    _need(w, (cout, seq * cin), name="w")
    _need_like(dpre, "dpre", (bsz, vsrc, cin), torch.float32, elu_y=elu_y)
    dx = _out(out, (bsz, vsrc, cin), dpre)
    if general or not spiral_conv_has_shape(CONV_BWD_DATA, seq, cin, cout):  # no instance: the general kernel
        _check_gen_limits(seq, cin, cout)
        call("cfsd_spiral_conv_gen_bwd_data", ptr(dpre), ptr(inv_ptr), ptr(inv_row), ptr(w), ptr(elu_y), ptr(dx),
             bsz, vsrc, rows, seq, cin, cout, stream_ptr())
        return dx
    ws, nb = _conv_ws(workspace, dpre.device, spiral_conv_workspace(bsz, vsrc, rows, seq, cin, cout))
    call("cfsd_spiral_conv_bwd_data", ptr(dpre), ptr(inv_ptr), ptr(inv_row), ptr(inv_head), ptr(w),
         ptr(elu_y), ptr(dx), ptr(ws), ctypes.c_size_t(nb), bsz, vsrc, rows, seq, cin, cout,
         stream_ptr())
    return dx


def spiral_conv_bwd_weight_workspace(bsz, rows, seq, cin, cout, general=False):
    if general or not spiral_conv_has_shape(CONV_BWD_WEIGHT, seq, cin, cout):
        return int(_abi.lib().cfsd_spiral_conv_gen_bwd_weight_workspace(bsz, rows, seq, cin, cout))
    return int(_abi.lib().cfsd_spiral_conv_bwd_weight_workspace(bsz, rows, seq, cin, cout))


def spiral_conv_bwd_weight(x, idx, dpre, dw, db, workspace, general=False):
    """dW/db of one SpiralConv.  With ``dw is db is None`` the reduction is
    deferred: the partials stay in ``workspace`` and a DeferredDw descriptor
    is returned for ``dw_reduce_batch`` (which must get the real dw/db).  A
    shape without a specialised instance takes the general kernel; its deferred
    slabs (:class:`DeferredGenDw`) are reduced by ``spiral_conv_gen_dw_reduce``
    or as an item of ``dw_reduce_batch``, which reduces them in a launch of
    their own before the batched one.  ``general``: as :func:`spiral_conv_fwd`."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _need(x, None, name="x")
    _need(dpre, (bsz, rows, cout), name="dpre")
    _need_dw_db(dw, db, cout, seq * cin)
    workspace, nbytes = _conv_ws(_need(workspace, None, name="workspace"), x.device,
                                 spiral_conv_bwd_weight_workspace(bsz, rows, seq, cin, cout, general))
    if general or not spiral_conv_has_shape(CONV_BWD_WEIGHT, seq, cin, cout):  # no instance: the general kernel
        _check_gen_limits(seq, cin, cout)
        call("cfsd_spiral_conv_gen_bwd_weight", ptr(x), ptr(idx), ptr(dpre), ptr(dw), ptr(db), ptr(workspace),
             ctypes.c_size_t(nbytes), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
        return DeferredGenDw(workspace, bsz, rows, seq, cin, cout) if dw is None else None
    call("cfsd_spiral_conv_bwd_weight", ptr(x), ptr(idx), ptr(dpre), ptr(dw), ptr(db),
         ptr(workspace), ctypes.c_size_t(nbytes), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return _deferred(dw, workspace, bsz, vsrc, rows, cin, cout, DW_PLAIN)


class DeferredDw:
    """Slab set left by a deferred weight-gradient call (see dw_reduce_batch)."""

    def __init__(self, workspace, batch, vsrc, rows, cin, cout, fused):
        self.workspace = workspace
        self.sizes = (batch, vsrc, rows, cin, cout, int(fused))

    def desc(self, dw, db):
        _need(dw, (self.sizes[4], 9 * self.sizes[3]), name="dw")
        _need(db, (self.sizes[4],), name="db")
        return _abi.DwSlabs(self.workspace.data_ptr(), dw.data_ptr(), db.data_ptr(), *self.sizes)


def _deferred(dw, workspace, bsz, vsrc, rows, cin, cout, code):
    """What a weight-gradient call returns for its dW: the reduction was
    deferred iff ``dw is None``, and then the slabs in ``workspace`` are
    described by the entry point's ``CFSD_DW_*`` code; None when it reduced."""
    return DeferredDw(workspace, bsz, vsrc, rows, cin, cout, code) if dw is None else None


def _with_dx(dx, d):
    """What a dx + dW call returns: ``dx``, or ``(dx, d)`` when it deferred the weight gradient."""
    return dx if d is None else (dx, d)


class DeferredGenDw:
    """Slab set left by a deferred general-shape weight gradient
    (``cfsd_spiral_conv_gen_bwd_weight`` with dw = db = NULL)."""

    def __init__(self, workspace, batch, rows, seq, cin, cout):
        self.workspace = workspace
        self.sizes = (batch, rows, seq, cin, cout)


def spiral_conv_gen_dw_reduce(d, dw, db):
    """Second stage of a deferred general-shape weight gradient: the slabs of
    ``d`` (:class:`DeferredGenDw`) summed into dw / db, bit-identical to the
    immediate form."""
    bsz, rows, seq, cin, cout = d.sizes
    _need(dw, (cout, seq * cin), name="dw")
    _need(db, (cout,), name="db")
    nbytes = d.workspace.numel() * d.workspace.element_size()
    call("cfsd_spiral_conv_gen_dw_reduce", ptr(d.workspace), ctypes.c_size_t(nbytes), ptr(dw), ptr(db), bsz, rows,
         seq, cin, cout, stream_ptr())


def dw_reduce_batch(items, adam=None):
    """Reduce several deferred weight gradients in ONE launch.
    ``items``: list of (DeferredDw, dw, db).  ``adam``: optional dict(param,
    grad, m, v, step, lr, beta1, beta2, eps, weight_decay, shadow) -- the Adam
    step over the whole flat buffers fused into the same launch (the items'
    dw/db must be views of ``grad``)."""
    # general-shape slab sets are not items of the batched launch: each is reduced into its
    # dw / db first, so with ``adam`` the batched launch's rest workgroups update those elements
    gen = [it for it in items if isinstance(it[0], DeferredGenDw)]
    if gen:
        for d, dw, db in gen:
            spiral_conv_gen_dw_reduce(d, dw, db)
        items = [it for it in items if not isinstance(it[0], DeferredGenDw)]
    if not items and adam is None:
        return
    arr = (_abi.DwSlabs * max(len(items), 1))(*[d.desc(dw, db) for d, dw, db in items])
    if adam is None:
        call("cfsd_dw_reduce_batch", arr, len(items), stream_ptr())
        return
    a = adam
    n = a["param"].numel()
    for t, nm in ((a["param"], "param"), (a["grad"], "grad"), (a["m"], "m"), (a["v"], "v")):
        _need(t, (n,), name=nm)
    _need(a["step"], (1,), torch.int32, "step")
    if a.get("shadow") is not None:
        _need(a["shadow"], (n,), torch.bfloat16, "shadow")
    call("cfsd_dw_reduce_batch_adam", arr, len(items), ptr(a["param"]), ptr(a["grad"]), ptr(a["m"]),
         ptr(a["v"]), ptr(a["step"]), ctypes.c_size_t(n), float(a["lr"]), float(a["beta1"]),
         float(a["beta2"]), float(a["eps"]), float(a["weight_decay"]), ptr(a.get("shadow")), stream_ptr())


def spiral_conv_bwd_workspace(bsz, vsrc, rows, seq, cin, cout):
    if spiral_conv_bwd_is_general(seq, cin, cout, dx=False):  # no fused launch, no dW instance: the general
        return spiral_conv_bwd_weight_workspace(bsz, rows, seq, cin, cout)  # dW slabs (the general dx needs none)
    # the library's own query; it also covers a specialised dW followed by the general dx
    return int(_abi.lib().cfsd_spiral_conv_bwd_workspace(bsz, vsrc, rows, seq, cin, cout))


def spiral_conv_bwd_paired(bsz, vsrc, rows, seq, cin, cout):
    """True when spiral_conv_bwd (with dx) runs dx and dW as one paired launch."""
    return bool(_abi.lib().cfsd_spiral_conv_bwd_paired(bsz, vsrc, rows, seq, cin, cout))


def spiral_conv_bwd(x, idx, dpre, inv, w, dw, db, dx=None, elu_y=None, workspace=None):
    """Fused dX (skipped when ``dx`` is None) + dW/db of one SpiralConv; same
    results as spiral_conv_bwd_data followed by spiral_conv_bwd_weight."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _need(x, None, name="x")
    _need(dpre, (bsz, rows, cout), name="dpre")
    inv_ptr, inv_row, inv_head = _need_inv(inv, vsrc, rows, seq)
    _need(w, (cout, seq * cin), name="w")
    _need_dw_db(dw, db, cout, seq * cin)
    _need_like(x, "x", (bsz, vsrc, cin), torch.float32, dx=dx, elu_y=elu_y)
    ws, nb = _conv_ws(workspace, x.device, spiral_conv_bwd_workspace(bsz, vsrc, rows, seq, cin, cout))
    if spiral_conv_bwd_is_general(seq, cin, cout, dx=dx is not None):  # the library refuses: two launches
        if dx is not None:
            spiral_conv_bwd_data(dpre, inv, w, vsrc, elu_y=elu_y, out=dx)
        d = spiral_conv_bwd_weight(x, idx, dpre, dw, db, ws)
        return _with_dx(dx, d)
    call("cfsd_spiral_conv_bwd", ptr(x), ptr(idx), ptr(dpre), ptr(inv_ptr), ptr(inv_row),
         ptr(inv_head), ptr(w), ptr(elu_y), ptr(dx), ptr(dw), ptr(db), ptr(ws), ctypes.c_size_t(nb),
         bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return _with_dx(dx, _deferred(dw, ws, bsz, vsrc, rows, cin, cout, DW_FUSED))


def spiral_conv_bwd_rowsub_workspace(bsz, vsrc, rows, seq, cin, cout):
    """0 when the shape has no row-subset backward (cin != 32)."""
    return int(_abi.lib().cfsd_spiral_conv_bwd_rowsub_workspace(bsz, vsrc, rows, seq, cin, cout))


def spiral_conv_bwd_rowsub(x, idx, dpre, flat, w, dw, db, dx, elu_y=None, workspace=None):
    """dX + dW/db of a conv evaluated on a row subset (an Enblock conv):
    dG = dpre.W at the kept rows, then the ascending-order gather-sum of dG
    through ``flat`` = ``topology.inverse_flat``'s (table, width)."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    # batch-major x, or vertex-major fp32 x (the fp32 step's E1: cfsd_spiral_conv_bwd_rowsub_x)
    _needl(x, None, "x", torch.float32)
    _need(dpre, (bsz, rows, cout), name="dpre")
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, seq * cin), name="w")
    _need_dw_db(dw, db, cout, seq * cin)
    if dx is None:
        raise ValueError("dx is required")
    _need_like(x, "x", (bsz, vsrc, cin), torch.float32, dx=dx, elu_y=elu_y)  # the source level's layout
    need = spiral_conv_bwd_rowsub_workspace(bsz, vsrc, rows, seq, cin, cout)
    if need == 0:
        raise ValueError(f"no row-subset backward for {cin} -> {cout} channels")
    ws, nb = _conv_ws(workspace, x.device, need)
    rest = (ptr(idx), ptr(dpre), ptr(table), width, ptr(w), ptr(elu_y), ptr(dx), ptr(dw), ptr(db), ptr(ws),
            ctypes.c_size_t(nb), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    if is_vm(x):
        call("cfsd_spiral_conv_bwd_rowsub_x", ptr(x), _st(x), *rest)
    else:
        call("cfsd_spiral_conv_bwd_rowsub", ptr(x), *rest)
    return _with_dx(dx, _deferred(dw, ws, bsz, vsrc, rows, cin, cout, DW_FUSED))  # slabs at the workspace start


def spiral_conv_bwd_data_rowsub_workspace(bsz, rows, seq, cin):
    return int(_abi.lib().cfsd_spiral_conv_bwd_data_rowsub_workspace(bsz, rows, seq, cin))


def spiral_conv_bwd_data_rowsub(dpre, flat, w, vsrc, elu_y=None, out=None, workspace=None):
    """dx of a row-subset conv (dG = dpre.W at the kept rows, then the
    ascending flat gather); ``out``/``elu_y`` fp32 or bf16 (bf16 path)."""
    bsz, rows, cout = dpre.shape
    cin = w.shape[1] // 9
    _need(dpre, None, name="dpre")
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, 9 * cin), name="w")
    _needl(out, (bsz, vsrc, cin), "out")
    _need_like(out, "out", (bsz, vsrc, cin), out.dtype, elu_y=elu_y)
    need = spiral_conv_bwd_data_rowsub_workspace(bsz, rows, 9, cin)
    if need == 0:
        raise ValueError(f"no row-subset backward for {cin} -> {cout} channels")
    ws, nb = _conv_ws(workspace, dpre.device, need)
    call("cfsd_spiral_conv_bwd_data_rowsub", ptr(dpre), ptr(table), width, ptr(w), ptr(elu_y), ptr(out),
         _st(out), ptr(ws), ctypes.c_size_t(nb), bsz, vsrc, rows, 9, cin, cout, stream_ptr())
    return out


def spiral_gather(x, idx, out=None):
    bsz, vsrc, rows, seq, cin = _conv_dims(x, idx)
    _need(x, None, name="x")
    g = _out(out, (bsz, rows, seq * cin), x)
    call("cfsd_spiral_gather", ptr(x), ptr(idx), ptr(g), bsz, vsrc, rows, seq, cin, stream_ptr())
    return g


# ------------------------------------------------------------------ pool / swap
def spmm(csr, x, m, elu_y=None, out=None, order=None, uniform=0, sched=None):
    """y[b, r] = g * sum_{k in row r} val[k] x[b, col[k]]   (Pool, model.py:50-55).
    ``order``: optional row schedule (a permutation of the rows by decreasing
    length, for matrices with long skewed rows); ``uniform``: every row holds
    exactly that many entries (``topology.uniform_rows``; no row_ptr walk);
    ``sched``: the CSR re-stored in a visiting order (``topology.scheduled_csr``,
    replaces ``csr``/``order``).  Same results bit for bit in every form."""
    row_ptr, col, val = csr
    bsz, n, c = x.shape
    _need(x, None, name="x")
    _need(row_ptr, (m + 1,), torch.int32, "row_ptr")
    _need(col, None, torch.int32, "col")
    _need(val, (col.numel(),), name="val")
    if elu_y is not None:
        _need(elu_y, (bsz, m, c), name="elu_y")
    y = _out(out, (bsz, m, c), x)
    if sched is not None:
        _spmm_sched_csr(sched, x, elu_y, y, bsz, m, n, c)
        return y
    if order is not None:
        _spmm_sched(row_ptr, col, val, order, x, elu_y, y, bsz, m, n, c)
        return y
    if uniform:
        _spmm_uniform(uniform, col, val, x, elu_y, y, bsz, m, n, c)
        return y
    call("cfsd_spmm_csr", ptr(row_ptr), ptr(col), ptr(val), ptr(x), ptr(elu_y), ptr(y), bsz, m, n,
         c, stream_ptr())
    return y


def _spmm_uniform(k, col, val, x, elu_y, y, bsz, m, n, c):
    """cfsd_spmm_uniform: every row holds exactly ``k`` entries."""
    if col.numel() != m * k:
        raise ValueError(f"uniform SpMM: {col.numel()} entries != {m} rows x {k}")
    call("cfsd_spmm_uniform", int(k), ptr(col), ptr(val), ptr(x), _st(x), ptr(elu_y), ptr(y), _st(y),
         bsz, m, n, c, stream_ptr())


def _spmm_sched_csr(sched, x, elu_y, y, bsz, m, n, c):
    """cfsd_spmm_sched_csr over a CSR stored in visiting order."""
    ptr_s, col_s, val_s, rows_s = sched
    _need(ptr_s, (m + 1,), torch.int32, "ptr_s")
    _need(rows_s, (m,), torch.int32, "rows_s")
    _need(col_s, None, torch.int32, "col_s")
    _need(val_s, (col_s.numel(),), name="val_s")
    call("cfsd_spmm_sched_csr", ptr(ptr_s), ptr(col_s), ptr(val_s), ptr(rows_s), ptr(x), _st(x), ptr(elu_y),
         ptr(y), _st(y), bsz, m, n, c, stream_ptr())


def _spmm_sched(row_ptr, col, val, order, x, elu_y, y, bsz, m, n, c):
    """cfsd_spmm_csr_sched: rows visited in ``order`` (``topology.row_schedule``)."""
    _need(order, (m,), torch.int32, "order")
    call("cfsd_spmm_csr_sched", ptr(row_ptr), ptr(col), ptr(val), ptr(order), ptr(x), _st(x),
         ptr(elu_y), ptr(y), _st(y), bsz, m, n, c, stream_ptr())


def swap_features(x_all, batch_idx, region_mask, key, bs, out=None):
    """``SwapFeatures.__call__`` (swap_batch_transform.py:13-42) on device."""
    n_meshes, nv, c = x_all.shape
    _need(x_all, None, name="x_all")
    _need(batch_idx, (bs,), torch.int32, "batch_idx")
    if region_mask is None or region_mask.dim() != 2:
        raise ValueError("region_mask [n_regions, nv] is required")
    _need(region_mask, (region_mask.shape[0], nv), torch.uint8, "region_mask")
    _need(key, (1,), torch.int32, "key")
    if out is not None and is_vm(out):  # vertex-major output (the fp32 step's level-0 input)
        _needl(out, (bs * bs, nv, c), "out", torch.float32)
        call("cfsd_swap_features_x", ptr(x_all), ptr(batch_idx), ptr(region_mask), ptr(key), ptr(out),
             _st(out), bs, nv, c, n_meshes, int(region_mask.shape[0]), stream_ptr())
        return out
    y = _out(out, (bs * bs, nv, c), x_all)
    call("cfsd_swap_features", ptr(x_all), ptr(batch_idx), ptr(region_mask), ptr(key), ptr(y), bs,
         nv, c, n_meshes, int(region_mask.shape[0]), stream_ptr())
    return y


def spiral_conv_fwd_in_swap(x_all, batch_idx, region_mask, key, bs, x_out, idx, w, bias, act, out):
    """:func:`swap_features` into ``x_out`` and the xyz input conv of the first
    Enblock (``out`` = act(conv(x_out)) at the rows of ``idx``) in one launch
    (``cfsd_spiral_conv_fwd_in_swap``): the conv gathers through the swap
    straight from ``x_all``.  ``x_out`` fp32, either layout; ``out`` fp32 or
    bf16, either layout."""
    n_meshes, nv, c = x_all.shape
    rows, seq = idx.shape
    cout = w.shape[0]
    _need(x_all, None, name="x_all")
    _need(batch_idx, (bs,), torch.int32, "batch_idx")
    if region_mask is None or region_mask.dim() != 2:
        raise ValueError("region_mask [n_regions, nv] is required")
    _need(region_mask, (region_mask.shape[0], nv), torch.uint8, "region_mask")
    _need(key, (1,), torch.int32, "key")
    _needl(x_out, (bs * bs, nv, c), "x_out", torch.float32)
    _need(idx, (rows, seq), torch.int32, "idx")
    _need(w, (cout, seq * c), name="w")
    _needl(out, (bs * bs, rows, cout), "out", out.dtype)
    call("cfsd_spiral_conv_fwd_in_swap", ptr(x_all), ptr(batch_idx), ptr(region_mask), ptr(key), bs, n_meshes,
         int(region_mask.shape[0]), ptr(x_out), _st(x_out), ptr(idx), ptr(w), ptr(bias), ptr(out), _st(out), nv, rows,
         c, cout, int(act), stream_ptr())
    return out


def spiral_conv_fwd_up_supported(bsz, rows, seq, cin, cout):
    return bool(_abi.lib().cfsd_spiral_conv_fwd_up_supported(bsz, rows, seq, cin, cout))


def spiral_conv_fwd_up(xc, comp, idx, w, bias, act, out, up_out=None):
    """SpiralDeblock forward (``model.py:80-82``) with Pool(up) fused into
    the gather: ``comp`` = the level's composite up table
    (``DeviceTopology.up_comp``); ``up_out`` receives Pool(xc, up) (the
    input the weight gradient reads), bit-identical to :func:`spmm`."""
    bsz, n_coarse, cin = xc.shape
    rows, seq = idx.shape
    cout = w.shape[0]
    _need(xc, None, name="xc")
    _need(idx, (rows, seq), torch.int32, "idx")
    _need(comp[0], (rows, seq, 3), torch.int32, "comp_col")
    _need(comp[1], (rows, seq, 3), torch.float32, "comp_val")
    _need(w, (cout, seq * cin), name="w")
    _need(out, (bsz, rows, cout), name="out")
    if up_out is not None:
        _need(up_out, (bsz, rows, cin), name="up_out")
    call("cfsd_spiral_conv_fwd_up", ptr(xc), ptr(comp[0]), ptr(comp[1]), ptr(idx), ptr(w), ptr(bias), ptr(out),
         ptr(up_out), bsz, n_coarse, rows, seq, cin, cout, int(act), stream_ptr())
    return out


def gather_meshes(x_all, batch_idx, bs, out=None):
    """The un-swapped batch of a ``swap_features: False`` configuration
    (``data_loading.py:38, 81-82``: MeshCollater without a feature swapper):
    ``out[b] = x_all[batch_idx[b]]`` on device (``cfsd_gather_meshes``)."""
    n_meshes, nv, c = x_all.shape
    _need(x_all, None, name="x_all")
    _need(batch_idx, (bs,), torch.int32, "batch_idx")
    if out is not None and is_vm(out):
        _needl(out, (bs, nv, c), "out", torch.float32)
        y = out
    else:
        y = _out(out, (bs, nv, c), x_all)
    call("cfsd_gather_meshes", ptr(x_all), ptr(batch_idx), ptr(y), _st(y), bs, nv, c, n_meshes, stream_ptr())
    return y


def spectral_blend(s1, s2, values, n_blend, out=None):
    """Augmentation coefficients s1 + v * (s2 - s1) on the first ``n_blend``
    spectral components (utils.py:256-267); s1/s2 [pairs, k, c], values [pairs, k]."""
    _need(s1, None, name="s1")
    if s1.dim() != 3:
        raise ValueError(f"s1: shape {tuple(s1.shape)}, expected [pairs, k, c]")
    p, k, c = s1.shape
    _need(s2, (p, k, c), name="s2")
    _need(values, (p, k), name="values")
    y = _out(out, (p, k, c), s1)
    call("cfsd_spectral_blend", ptr(s1), ptr(s2), ptr(values), ptr(y), p, k, c, int(n_blend), stream_ptr())
    return y


def normalize(x, mean, std, out=None):
    """``(x - mean) / std`` per vertex (data_loading.py:259-260), bit-exact."""
    _need(x, None, name="x")
    if x.dim() != 3:
        raise ValueError(f"x: shape {tuple(x.shape)}, expected [n_meshes, nv, c]")
    n, nv, c = x.shape
    _need(mean, (nv, c), name="mean")
    _need(std, (nv, c), name="std")
    y = _out(out, (n, nv, c), x)
    call("cfsd_normalize", ptr(x), ptr(mean), ptr(std), ptr(y), n, nv, c, stream_ptr())
    return y


def elu_bwd(dy, y, out=None):
    _need(dy, None, name="dy")
    _need(y, tuple(dy.shape), name="y")
    dx = _out(out, tuple(dy.shape), dy)
    call("cfsd_elu_bwd", ptr(dy), ptr(y), ptr(dx), ctypes.c_size_t(dy.numel()), stream_ptr())
    return dx


# ------------------------------------------------------------------ dense
def linear_workspace(m, k, n):
    return int(_abi.lib().cfsd_linear_workspace(m, k, n))


def _ws(workspace, need):
    if need == 0:
        return None, 0
    if workspace is None:
        raise ValueError(f"linear: workspace of {need} bytes required")
    nbytes = workspace.numel() * workspace.element_size()
    if nbytes < need:
        raise ValueError(f"linear: workspace {nbytes} < {need} bytes")
    return workspace, nbytes


def linear_fwd(x, w, b, out=None, workspace=None):
    m, k = x.shape
    n = w.shape[0]
    _need(x, None, name="x")
    _need(w, (n, k), name="w")
    if b is not None:
        _need(b, (n,), name="b")
    y = _out(out, (m, n), x)
    if workspace is None and linear_workspace(m, k, n):
        workspace = torch.empty(linear_workspace(m, k, n) // 4, device=x.device)
    ws, nb = _ws(workspace, linear_workspace(m, k, n))
    call("cfsd_linear_fwd", ptr(x), ptr(w), ptr(b), ptr(y), ptr(ws), ctypes.c_size_t(nb), m, k, n,
         stream_ptr())
    return y


def linear_bwd(x, w, dy, dx=None, dw=None, db=None, elu_y=None, accumulate=False, workspace=None):
    m, n = dy.shape
    k = w.shape[1] if w is not None else x.shape[1]
    _need(dy, None, name="dy")
    if dx is not None:
        _need(dx, (m, k), name="dx")
        _need(w, (n, k), name="w")
    if dw is not None:
        _need(dw, (n, k), name="dw")
        _need(x, (m, k), name="x")
    if db is not None:
        _need(db, (n,), name="db")
    if elu_y is not None:
        _need(elu_y, (m, k), name="elu_y")
    need = linear_workspace(m, k, n) if dx is not None else 0
    if workspace is None and need:
        workspace = torch.empty(need // 4, device=dy.device)
    ws, nb = _ws(workspace, need)
    call("cfsd_linear_bwd", ptr(x), ptr(w), ptr(dy), ptr(elu_y), ptr(dx), ptr(dw), ptr(db),
         ptr(ws), ctypes.c_size_t(nb), m, k, n, int(accumulate), stream_ptr())


# ------------------------------------------------------------------ losses
def recon_lap_blocks(bsz, nv):
    return int(_abi.lib().cfsd_recon_lap_blocks(bsz, nv))


def _loss_layout(*ts):
    """Storage flag of the loss operands: all batch-major or all vertex-major."""
    vm = [is_vm(t) for t in ts]
    if any(vm) and not all(vm):
        raise ValueError("loss operands must share one layout (batch-major or vertex-major)")
    for t in ts:
        _needl(t, tuple(ts[0].shape), "loss operand", torch.float32)
    return VM if vm[0] else 0


def recon_lap_fwd(pred, gt, lap_csr, unit, partials):
    bsz, nv, c = pred.shape
    lay = _loss_layout(pred, gt, unit)
    _need(partials, (2 * recon_lap_blocks(bsz, nv),), name="partials")
    _need(lap_csr[0], (nv + 1,), torch.int32, "l_ptr")
    call("cfsd_recon_lap_fwd_x", ptr(pred), ptr(gt), ptr(lap_csr[0]), ptr(lap_csr[1]),
         ptr(lap_csr[2]), ptr(unit), ptr(partials), bsz, nv, c, lay, stream_ptr())


def recon_lap_bwd(pred, gt, unit, lapT_csr, dpred, w_rec, w_lap):
    bsz, nv, c = pred.shape
    lay = _loss_layout(pred, gt, unit, dpred)
    _need(lapT_csr[0], (nv + 1,), torch.int32, "lt_ptr")
    call("cfsd_recon_lap_bwd_x", ptr(pred), ptr(gt), ptr(unit), ptr(lapT_csr[0]),
         ptr(lapT_csr[1]), ptr(lapT_csr[2]), ptr(dpred), bsz, nv, c, float(w_rec), float(w_lap), lay,
         stream_ptr())


def recon_lap_bwd_finalize(pred, gt, unit, lapT_csr, dpred, w_rec, w_lap, partials, terms, out, acc,
                           w_kl, w_lc):
    """recon_lap_bwd + loss_finalize in one launch (the last workgroup
    finalises the losses of the preceding recon_lap_fwd)."""
    bsz, nv, c = pred.shape
    lay = _loss_layout(pred, gt, unit, dpred)
    _need(lapT_csr[0], (nv + 1,), torch.int32, "lt_ptr")
    _need(partials, (2 * recon_lap_blocks(bsz, nv),), name="partials")
    _need(terms, (2,), name="terms")
    _need(out, (5,), name="out")
    if acc is not None:
        _need(acc, (6,), name="acc")
    call("cfsd_recon_lap_bwd_finalize_x", ptr(pred), ptr(gt), ptr(unit), ptr(lapT_csr[0]),
         ptr(lapT_csr[1]), ptr(lapT_csr[2]), ptr(dpred), bsz, nv, c, float(w_rec), float(w_lap),
         ptr(partials), partials.numel() // 2, ptr(terms), ptr(out), ptr(acc), float(w_kl),
         float(w_lc), lay, stream_ptr())


def latent_fwd(mulv, eps, key, z, dlat, terms, latent, region_size, train, is_vae, sigmoid,
               w_kl, w_lc, eta1, eta2):
    bsz = z.shape[0]
    _need(mulv, (bsz, 2 * latent if is_vae else latent), name="mulv")
    _need(z, (bsz, latent), name="z")
    _need(dlat, (bsz, 3 * latent), name="dlat")
    _need(terms, (2,), name="terms")
    if eps is not None:
        _need(eps, (bsz, latent), name="eps")
    if key is not None:
        _need(key, (1,), torch.int32, "key")
    call("cfsd_latent_fwd", ptr(mulv), ptr(eps), ptr(key), ptr(z), ptr(dlat), ptr(terms), bsz,
         latent, region_size, int(train), int(is_vae), int(sigmoid), float(w_kl), float(w_lc),
         float(eta1), float(eta2), stream_ptr())


def latent_linear_fwd_supported(batch, latent, n):
    return bool(_abi.lib().cfsd_latent_linear_fwd_supported(int(batch), int(latent), int(n)))


def latent_linear_fwd(mulv, eps, key, z, dlat, terms, latent, region_size, train, is_vae, sigmoid,
                      w_kl, w_lc, eta1, eta2, w, bias, out):
    """latent_fwd, then the decoder Linear out = z w^T + bias, in one launch
    (cfsd_latent_linear_fwd: z, dlat, out bit-identical to the two calls)."""
    bsz = z.shape[0]
    n = w.shape[0]
    _need(mulv, (bsz, 2 * latent if is_vae else latent), name="mulv")
    _need(z, (bsz, latent), name="z")
    _need(dlat, (bsz, 3 * latent), name="dlat")
    _need(terms, (2,), name="terms")
    _need(w, (n, latent), name="w")
    _need(out, (bsz, n), name="out")
    if bias is not None:
        _need(bias, (n,), name="bias")
    if eps is not None:
        _need(eps, (bsz, latent), name="eps")
    if key is not None:
        _need(key, (1,), torch.int32, "key")
    call("cfsd_latent_linear_fwd", ptr(mulv), ptr(eps), ptr(key), ptr(z), ptr(dlat), ptr(terms), bsz,
         latent, region_size, int(train), int(is_vae), int(sigmoid), float(w_kl), float(w_lc),
         float(eta1), float(eta2), ptr(w), ptr(bias), ptr(out), n, stream_ptr())


def latent_bwd(mulv, eps, z, dz_dec, dlat, dmulv, latent, train, is_vae, sigmoid):
    """``dz_dec`` [B, latent], or [parts, B, latent] partial products (summed
    in part order: cfsd_latent_bwd_parts)."""
    if dz_dec is None or dz_dec.dim() not in (2, 3):
        raise ValueError("dz_dec must be [B, latent] or [parts, B, latent]")
    bsz = dz_dec.shape[-2]
    _need(mulv, (bsz, 2 * latent if is_vae else latent), name="mulv")
    _need(dmulv, tuple(mulv.shape), name="dmulv")
    _need(dlat, (bsz, 3 * latent), name="dlat")
    if eps is not None:
        _need(eps, (bsz, latent), name="eps")
    # z is required by the sigmoid AE alone (zval * (1 - zval)); when given it is checked in every mode
    if z is not None or (sigmoid and not is_vae):
        _need(z, (bsz, latent), name="z")
    if dz_dec.dim() == 3:
        parts = dz_dec.shape[0]
        _need(dz_dec, (parts, bsz, latent), name="dz_parts")
        call("cfsd_latent_bwd_parts", ptr(mulv), ptr(eps), ptr(z), ptr(dz_dec), parts, ptr(dlat),
             ptr(dmulv), bsz, latent, int(train), int(is_vae), int(sigmoid), stream_ptr())
        return
    _need(dz_dec, (bsz, latent), name="dz_dec")
    call("cfsd_latent_bwd", ptr(mulv), ptr(eps), ptr(z), ptr(dz_dec), ptr(dlat), ptr(dmulv), bsz,
         latent, int(train), int(is_vae), int(sigmoid), stream_ptr())


BN_SYNC_INTS = _H["CFSD_BN_SYNC_INTS"]  # cfsd_bottleneck_bwd's counters and flags (19 x one 128-B line)
BN_SYNC_ERR = _H["CFSD_BN_SYNC_ERR"]    # the sticky timed-out-wait word inside them


def bottleneck_exchange_floats(batch, latent, nd, ne):
    """Size of cfsd_bottleneck_bwd's exchange workspace (device floats)."""
    return int(_abi.lib().cfsd_bottleneck_bwd_exchange_floats(batch, latent, nd, ne))


def bottleneck_check(sync):
    """Raise CfsdError if any cfsd_bottleneck_bwd launch that used ``sync``
    gave up waiting (its values are then wrong).  Reads one device int (a
    host sync): call it at a cadence, e.g. once per epoch, not per step."""
    err = int(sync[BN_SYNC_ERR].item())
    if err:
        raise _abi.CfsdError(f"cfsd_bottleneck_bwd: a wait timed out (roles {err:#x}); the step's "
                             f"bottleneck gradients are invalid")


def bottleneck_bwd(up_csr, g, z, wd, exchange, dwd, dbd, mulv, eps, dlat, dmulv, is_vae, sigmoid, xe, we, dxe,
                   dwe, dbe, sync, elu_y=None, accumulate=False, train=True):
    """The bottleneck backward in one launch (``cfsd_bottleneck_bwd``): the
    coarsest Pool(up) transpose over ``g`` [B, n_up, cup] (``up_csr`` =
    (row_ptr, col, val), plain per-row order), the decoder Linear backward
    (``wd`` [nd, latent]), the latent head backward (:func:`latent_bwd`) and
    the encoder Linear backward (:func:`linear_bwd` with ``xe`` [B, ke],
    ``we`` [ne, ke], dy = ``dmulv``).  ``exchange``: a device float buffer of
    :func:`bottleneck_exchange_floats` (the launch's line-exclusive hand-off
    area); ``sync``: BN_SYNC_INTS zeroed device int32, left zeroed (a timed-out
    wait sets ``sync[BN_SYNC_ERR]``: :func:`bottleneck_check`)."""
    row_ptr, col, val = up_csr
    bsz, n_up, cup = g.shape
    _need(g, None, name="g")
    if is_vm(g):
        raise ValueError("g must be batch-major")
    m, lat = z.shape
    nd, kd = wd.shape
    ne, ke = we.shape
    if kd != lat or m != bsz or nd % cup:
        raise ValueError(f"bottleneck_bwd: z {tuple(z.shape)}, wd {tuple(wd.shape)}, g {tuple(g.shape)}")
    _need(row_ptr, (nd // cup + 1,), torch.int32, "up_ptr")
    _need(col, None, torch.int32, "up_col")
    _need(val, (col.numel(),), name="up_val")
    _need(z, (m, lat), name="z")
    _need(exchange, (bottleneck_exchange_floats(m, lat, nd, ne),), name="exchange")
    _need(dwd, (nd, lat), name="dwd")
    _need(dbd, (nd,), name="dbd")
    _need(dmulv, tuple(mulv.shape), name="dmulv")
    _need(xe, (m, ke), name="xe")
    _need(dxe, (m, ke), name="dxe")
    if elu_y is not None:
        _need(elu_y, (m, ke), name="elu_y")
    _need(dwe, (ne, ke), name="dwe")
    _need(dbe, (ne,), name="dbe")
    _need(sync, (BN_SYNC_INTS,), torch.int32, "sync")
    call("cfsd_bottleneck_bwd", ptr(row_ptr), ptr(col), ptr(val), ptr(g), n_up, cup, ptr(z), ptr(wd), ptr(exchange),
         ptr(dwd), ptr(dbd), nd, ptr(mulv), ptr(eps), ptr(dlat), ptr(dmulv), int(train), int(is_vae), int(sigmoid),
         ptr(xe), ptr(we), ptr(elu_y), ptr(dxe), ptr(dwe), ptr(dbe), ke, ne, int(accumulate), ptr(sync), m, lat,
         stream_ptr())


def linear_bwd_split_parts(n):
    return int(_abi.lib().cfsd_linear_bwd_split_parts(n))


def linear_bwd_split(x, w, dy, dx_parts, dw, db):
    """Decoder-Linear backward in one launch: dW/db and dx as partial
    products over 64-row slices of W (``dx_parts`` [parts, m, k], summed by
    :func:`latent_bwd` with ``n_parts``)."""
    m, k = x.shape
    n = dy.shape[1]
    _need(x, (m, k), name="x")
    _need(w, (n, k), name="w")
    _need(dy, (m, n), name="dy")
    _need(dx_parts, (linear_bwd_split_parts(n), m, k), name="dx_parts")
    _need(dw, (n, k), name="dw")
    _need(db, (n,), name="db")
    call("cfsd_linear_bwd_split", ptr(x), ptr(w), ptr(dy), ptr(dx_parts), ptr(dw), ptr(db), m, k, n,
         stream_ptr())


def loss_finalize(partials, terms, out, acc, bsz, nv, c, w_kl, w_lc, w_lap):
    _need(partials, (2 * recon_lap_blocks(bsz, nv),), name="partials")
    _need(terms, (2,), name="terms")
    _need(out, (5,), name="out")
    if acc is not None:
        _need(acc, (6,), name="acc")
    call("cfsd_loss_finalize", ptr(partials), partials.numel() // 2, ptr(terms), ptr(out),
         ptr(acc), bsz, nv, c, float(w_kl), float(w_lc), float(w_lap), stream_ptr())


# ------------------------------------------------------------------ optimiser
def adam(param, grad, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
         shadow=None):
    """Adam over the flat fp32 buffers; ``shadow`` (bf16, same length) also
    receives the updated parameters (the bf16 path's weight copy)."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (m, "m"), (v, "v")):
        _need(t, (n,), name=nm)
    _need(step, (1,), torch.int32, "step")
    if shadow is not None:
        _need(shadow, (n,), torch.bfloat16, "shadow")
    call("cfsd_adam", ptr(param), ptr(grad), ptr(m), ptr(v), ptr(step), ctypes.c_size_t(n),
         float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), ptr(shadow),
         stream_ptr())


def adam_scaled(param, grad, m, v, step, grad_scale, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                shadow=None):
    """``scale(grad, grad_scale)`` then :func:`adam` in one launch (the
    data-parallel step's 1/world averaging folded into the update); ``grad``
    receives the scaled gradient."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (m, "m"), (v, "v")):
        _need(t, (n,), name=nm)
    _need(step, (1,), torch.int32, "step")
    if shadow is not None:
        _need(shadow, (n,), torch.bfloat16, "shadow")
    call("cfsd_adam_scaled", ptr(param), ptr(grad), ptr(m), ptr(v), ptr(step), ctypes.c_size_t(n),
         float(grad_scale), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), ptr(shadow),
         stream_ptr())


def step_begin(counter, seed, eps=None, key=None, n_regions=0, batch_idx=None, bs=0,
               n_batches=0, perm=None, adam_step=None, n_items=None, shuffle=False):
    """Per-step device bookkeeping (``cfsd_step_begin``): counter, swap key,
    VAE noise, the epoch-shuffled drop_last batch and Adam's t.  ``perm``
    (optional, int32) maps the ``n_items`` shuffled positions to dataset rows;
    its length and range are the caller's contract (validated once by
    ``engine.ResidentData``), not re-checked per step."""
    _need(counter, (1,), torch.int32, "counter")
    if adam_step is not None:
        _need(adam_step, (1,), torch.int32, "adam_step")
    if eps is not None:
        _need(eps, None, name="eps")
    if key is not None:
        _need(key, (1,), torch.int32, "key")
    if batch_idx is not None:
        _need(batch_idx, (bs,), torch.int32, "batch_idx")
        if n_items is None:
            n_items = perm.numel() if perm is not None else n_batches * bs
        if perm is not None:
            _need(perm, None, torch.int32, "perm")
            if perm.numel() < n_items:
                raise ValueError(f"perm has {perm.numel()} entries < n_items {n_items}")
        if n_items < n_batches * bs:
            raise ValueError(f"n_items {n_items} < n_batches {n_batches} x bs {bs}")
    call("cfsd_step_begin", ptr(counter), ctypes.c_ulonglong(seed), ptr(eps),
         eps.numel() if eps is not None else 0, ptr(key), n_regions, ptr(batch_idx), bs,
         n_batches, ptr(perm), int(n_items or 0), int(bool(shuffle)), ptr(adam_step), stream_ptr())


def scale(y, alpha):
    _need(y, None, name="y")
    call("cfsd_scale", ptr(y), ctypes.c_size_t(y.numel()), float(alpha), stream_ptr())


# ------------------------------------------------------------------ evaluation
def vertex_errors(out, gt, to_mm=89.11, mean=None, std=None, want_l1=False, want_mesh_mean=False):
    """``ModelManager.compute_vertex_errors`` (``model_manager.py:395-400``) on
    device: ``sqrt(sum_c (out - gt)^2) * to_mm`` per vertex, ``[B, V]``.

    ``mean``/``std`` ``[V, 3]`` un-normalise both inputs first
    (``Tester._unnormalize_verts``, ``test.py:81-84``).  ``want_l1`` also
    returns the per-vertex L1 ``sum_c |out - gt|``; ``want_mesh_mean`` the
    per-mesh mean used by ``Tester.reconstruction_errors`` (``test.py:297``).
    Returns ``err`` or a tuple ``(err, l1?, mesh_mean?)``."""
    _need(out, None, name="out")
    if out.dim() != 3 or out.shape[-1] != 3:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [B, V, 3]")
    bsz, nv = int(out.shape[0]), int(out.shape[1])
    _need(gt, tuple(out.shape), name="gt")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is not None:
        _need(mean, (nv, 3), name="mean")
        _need(std, (nv, 3), name="std")
    err = torch.empty((bsz, nv), dtype=torch.float32, device=out.device)
    l1 = torch.empty_like(err) if want_l1 else None
    mm = torch.empty((bsz,), dtype=torch.float32, device=out.device) if want_mesh_mean else None
    call("cfsd_vertex_errors", ptr(out), ptr(gt), ptr(mean), ptr(std), ptr(err), ptr(l1),
         ptr(mm), bsz, nv, float(to_mm), stream_ptr())
    if not (want_l1 or want_mesh_mean):
        return err
    return (err,) + ((l1,) if want_l1 else ()) + ((mm,) if want_mesh_mean else ())


RM_MAX_REGIONS, RM_THREADS = _H["CFSD_RM_MAX_REGIONS"], _H["CFSD_RM_THREADS"]


def group_vertex_errors(frames, n, to_mm=89.11, mean=None, std=None):
    """Distance of every frame of a traversal to its group's first frame
    (``Tester.latent_traversals``, ``test.py:157-158``: ``compute_vertex_errors``
    against ``gen_verts[0].expand(...)``) for ``G`` groups of ``n`` consecutive
    frames at once: ``frames`` ``[G*n, V, 3]`` -> ``err`` ``[G*n, V]``, bit-equal
    to :func:`vertex_errors` on the expanded first frames, which are read in
    place.  ``mean``/``std`` ``[V, 3]`` un-normalise first."""
    _need(frames, None, name="frames")
    if frames.dim() != 3 or frames.shape[-1] != 3:
        raise ValueError(f"frames: shape {tuple(frames.shape)}, expected [G*n, V, 3]")
    total, nv = int(frames.shape[0]), int(frames.shape[1])
    n = int(n)
    if n < 1 or total < 1 or nv < 1 or total % n:
        raise ValueError(f"{total} frames of {nv} vertices do not form groups of n={n}")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is not None:
        _need(mean, (nv, 3), name="mean")
        _need(std, (nv, 3), name="std")
    err = torch.empty((total, nv), dtype=torch.float32, device=frames.device)
    call("cfsd_group_vertex_errors", ptr(frames), ptr(mean), ptr(std), ptr(err), total // n, n, nv, float(to_mm),
         stream_ptr())
    return err


def region_means_depth(length):
    """``CFSD_RM_DEPTH``: the longest chain of additions one term of a list of
    ``length`` entries passes through in :func:`region_means`, plus one for
    the division."""
    return -(-int(length) // RM_THREADS) + 9


def region_means(values, region_csr):
    """Per-region mean of a per-vertex quantity (``test.py:208-215``):
    ``values`` ``[rows, V]``, ``region_csr`` a :class:`topology.RegionCSR`
    (``DeviceTopology.region_csr``) -> ``[rows, R]``, in a fixed summation
    order per (row, region) (``include/cfsd.h``)."""
    _need(values, None, name="values")
    if values.dim() != 2 or values.shape[0] < 1:
        raise ValueError(f"values: shape {tuple(values.shape)}, expected [rows >= 1, V]")
    rows, nv = int(values.shape[0]), int(values.shape[1])
    if nv != region_csr.nv:
        raise ValueError(f"values: {nv} columns, the regions index {region_csr.nv} vertices")
    n_regions = region_csr.n_regions
    if not 1 <= n_regions <= RM_MAX_REGIONS:
        raise ValueError(f"{n_regions} regions: 1..{RM_MAX_REGIONS} are supported")
    _need(region_csr.idx, (region_csr.nnz,), torch.int32, "region_csr.idx")
    if region_csr.idx.device != values.device:
        raise ValueError(f"region_csr is on {region_csr.idx.device}, values on {values.device}")
    out = torch.empty((rows, n_regions), dtype=torch.float32, device=values.device)
    call("cfsd_region_means", ptr(values), region_csr.ptr_host.ctypes.data_as(ctypes.c_void_p), ptr(region_csr.idx),
         ptr(out), rows, nv, n_regions, stream_ptr())
    return out


def reconstruction_error_stats(mesh_means):
    """The summary of ``Tester.reconstruction_errors`` (``test.py:298-301``)
    over the concatenated per-mesh means (device tensor, torch reductions)."""
    return {"mean": torch.mean(mesh_means).item(), "median": torch.median(mesh_means).item(),
            "max": torch.max(mesh_means).item(), "std": torch.std(mesh_means).item()}


# ------------------------------------------------------------------ classifiers
CLS_MAX_D = _H["CFSD_CLS_MAX_D"]  # widest column window of cfsd_class_stats / cfsd_discriminant_scores
CLS_MAX_CLASSES = _H["CFSD_CLS_MAX_CLASSES"]
MLP_MAX_LAYERS, MLP_MAX_WIDTH = _H["CFSD_MLP_MAX_LAYERS"], _H["CFSD_MLP_MAX_WIDTH"]
MLP_MAX_BS = _H["CFSD_MLP_MAX_BS"]


def _window(z, cols, name="z"):
    """``z`` [n, ld] and the column window ``cols = (col0, d)`` (default: all)."""
    _need(z, None, name=name)
    if z.dim() != 2 or z.shape[0] < 1:
        raise ValueError(f"{name}: shape {tuple(z.shape)}, expected [N >= 1, D]")
    n, ld = int(z.shape[0]), int(z.shape[1])
    col0, d = (0, ld) if cols is None else (int(cols[0]), int(cols[1]))
    if col0 < 0 or d < 1 or col0 + d > ld:
        raise ValueError(f"columns [{col0}, {col0 + d}) outside [0, {ld})")
    if d > CLS_MAX_D:
        raise ValueError(f"{d} columns: at most {CLS_MAX_D} are supported")
    return n, ld, col0, d


def class_stats(z, label, n_classes, cols=None, workspace=None):
    """Per-class count, mean and centred scatter (``cfsd_class_stats``) of the
    columns ``cols = (col0, d)`` of ``z`` ``[n, ld]``; ``label`` ``[n]`` int32,
    a label outside ``[0, n_classes)`` drops its row.  Returns ``(count [C]
    int32, mean [C, d], scatter [C, d, d])`` on the device."""
    n, ld, col0, d = _window(z, cols)
    _need(label, (n,), torch.int32, "label")
    if not 1 <= n_classes <= CLS_MAX_CLASSES:
        raise ValueError(f"{n_classes} classes: 1..{CLS_MAX_CLASSES} are supported")
    need = int(_abi.lib().cfsd_class_stats_workspace(n, d, n_classes))
    workspace, nbytes = _conv_ws(workspace, z.device, need)
    count = torch.empty((n_classes,), dtype=torch.int32, device=z.device)
    mean = torch.empty((n_classes, d), dtype=torch.float32, device=z.device)
    scatter = torch.empty((n_classes, d, d), dtype=torch.float32, device=z.device)
    call("cfsd_class_stats", ptr(z), ptr(label), ptr(count), ptr(mean), ptr(scatter), ptr(workspace),
         ctypes.c_size_t(nbytes), n, ld, col0, d, n_classes, stream_ptr())
    return count, mean, scatter


def discriminant_scores(z, mean, whiten, offset, cols=None, want_maha2=False, want_scores=True, want_pred=True):
    """``cfsd_discriminant_scores``: per row of the column window of ``z`` and
    class c, ``maha2 = |(z - mean_c) whiten_c|^2`` and ``scores = -0.5 maha2 +
    offset_c``; ``pred`` the arg max (lowest class on ties).  ``whiten``
    ``[C, d, d]`` (QDA) or ``[1, d, d]`` (shared, LDA).  Returns the dict of
    the outputs asked for."""
    n, ld, col0, d = _window(z, cols)
    _need(mean, None, name="mean")
    c = int(mean.shape[0])
    _need(mean, (c, d), name="mean")
    _need(offset, (c,), name="offset")
    _need(whiten, None, name="whiten")
    if whiten.dim() != 3 or whiten.shape[0] not in (1, c) or tuple(whiten.shape[1:]) != (d, d):
        raise ValueError(f"whiten: shape {tuple(whiten.shape)}, expected [{c} or 1, {d}, {d}]")
    if not 1 <= c <= CLS_MAX_CLASSES:
        raise ValueError(f"{c} classes: 1..{CLS_MAX_CLASSES} are supported")
    out = {}
    if want_maha2:
        out["maha2"] = torch.empty((n, c), dtype=torch.float32, device=z.device)
    if want_scores:
        out["scores"] = torch.empty((n, c), dtype=torch.float32, device=z.device)
    if want_pred:
        out["pred"] = torch.empty((n,), dtype=torch.int32, device=z.device)
    call("cfsd_discriminant_scores", ptr(z), ptr(mean), ptr(whiten), ptr(offset), ptr(out.get("maha2")),
         ptr(out.get("scores")), ptr(out.get("pred")), n, ld, col0, d, c, int(whiten.shape[0]), stream_ptr())
    return out


def mlp_dims(dims):
    """The host width array of the MLP entry points, validated."""
    dims = [int(v) for v in dims]
    if not 2 <= len(dims) <= MLP_MAX_LAYERS + 1:
        raise ValueError(f"{len(dims) - 1} layers: 1..{MLP_MAX_LAYERS} are supported")
    if min(dims) < 1 or max(dims) > MLP_MAX_WIDTH:
        raise ValueError(f"widths {dims}: 1..{MLP_MAX_WIDTH} are supported")
    return dims, (ctypes.c_int * len(dims))(*dims)


def mlp_param_count(dims):
    return sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))


def mlp_forward(z, params, dims):
    """The reference ``MLPClassifier`` (``model.py:191-203``: a ReLU after
    every Linear, the last included) in one launch (``cfsd_mlp_fwd``):
    ``z`` ``[n, dims[0]]``, ``params`` the flat fp32 buffer in ``state_dict``
    order.  Returns ``(logits [n, dims[-1]], pred [n] int32)``."""
    dims, cdims = mlp_dims(dims)
    _need(z, None, name="z")
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] != dims[0]:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [N >= 1, {dims[0]}]")
    _need(params, (mlp_param_count(dims),), name="params")
    n = int(z.shape[0])
    logits = torch.empty((n, dims[-1]), dtype=torch.float32, device=z.device)
    pred = torch.empty((n,), dtype=torch.int32, device=z.device)
    call("cfsd_mlp_fwd", ptr(z), ptr(params), ptr(logits), ptr(pred), cdims, len(dims) - 1, n, stream_ptr())
    return logits, pred


def mlp_workspace(dims, bs):
    dims, cdims = mlp_dims(dims)
    return int(_abi.lib().cfsd_mlp_workspace(cdims, len(dims) - 1, int(bs)))


def mlp_train_steps(z, label, class_weight, params, m, v, step, acc, dims, bs, n_steps, row0=0, train=True, lr=1e-4,
                    beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, workspace=None, dw_out=None):
    """``n_steps`` consecutive steps of ``mlp_classifier_epoch``
    (``model_manager.py:428-446``) over the rows ``[row0 + t bs, +bs)`` of
    ``z`` / ``label`` in ONE call (``cfsd_mlp_train_steps``: two launches per
    step).  ``acc`` ``[3]`` gains ``{loss, acc, 1}`` per step; ``step`` (int32
    device scalar) is Adam's t.  ``train=False`` is the validation epoch:
    parameters, moments and ``step`` stay untouched."""
    dims, cdims = mlp_dims(dims)
    _need(z, None, name="z")
    if z.dim() != 2 or z.shape[1] != dims[0]:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [N, {dims[0]}]")
    n_rows = int(z.shape[0])
    _need(label, (n_rows,), torch.int32, "label")
    _need(class_weight, (dims[-1],), name="class_weight")
    if not 1 <= bs <= MLP_MAX_BS:
        raise ValueError(f"batch size {bs}: 1..{MLP_MAX_BS} are supported")
    if n_steps < 0 or row0 < 0 or row0 + n_steps * bs > n_rows:
        raise ValueError(f"rows [{row0}, +{n_steps} x {bs}) outside [0, {n_rows})")
    n = mlp_param_count(dims)
    _need(params, (n,), name="params")
    _need(acc, (3,), name="acc")
    nbytes = 0
    if train:
        _need(m, (n,), name="m")
        _need(v, (n,), name="v")
        _need(step, (1,), torch.int32, "step")
        workspace, nbytes = _conv_ws(workspace, z.device, mlp_workspace(dims, bs))
    if dw_out is not None:
        _need(dw_out, (n,), name="dw_out")
    call("cfsd_mlp_train_steps", ptr(z), ptr(label), ptr(class_weight), ptr(params), ptr(m), ptr(v), ptr(step),
         ptr(acc), ptr(workspace) if train else None, ctypes.c_size_t(nbytes), ptr(dw_out), cdims, len(dims) - 1,
         n_rows, int(row0), int(bs), int(n_steps), int(bool(train)), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), stream_ptr())


def mlp_head_step(z, batch_idx, label_table, class_weight, params, acc, dims, bs, row_stride=1, train=True, m=None,
                  v=None, step=None, dlat=None, w_cls=1.0, dw_out=None, workspace=None, lr=1e-4, beta1=0.9,
                  beta2=0.999, eps=1e-8, weight_decay=0.0):
    """The MLP classifier as a head of the VAE step (``cfsd_mlp_head_step``,
    ``mlp_training_type: end2end``, ``model_manager.py:295-318``): two
    launches.  Row ``i < bs`` of the batch is row ``i * row_stride`` of ``z``
    ``[rows, >= dims[0]]`` (``row_stride = bs + 1``: the diagonal of a swapped
    group); its label is ``label_table[batch_idx[i]]`` (both int32).  ``acc``
    ``[3]`` gains ``{loss, accuracy, 1}``.  ``train``: ``step`` += 1, ``w_cls *
    dz`` is added to the first ``dims[0]`` columns of the same rows of ``dlat``
    ``[rows, ld]``, and the parameters' gradient (times ``w_cls``) either
    drives Adam in place (``m``, ``v`` given; ``dw_out`` optional) or is only
    written to ``dw_out`` (``m = v = None``).  ``train=False``: loss and
    accuracy only."""
    dims, cdims = mlp_dims(dims)
    bs, row_stride = int(bs), int(row_stride)
    if not 1 <= bs <= MLP_MAX_BS:
        raise ValueError(f"batch size {bs}: 1..{MLP_MAX_BS} are supported")
    if row_stride < 1:
        raise ValueError(f"row_stride {row_stride} < 1")
    _need(z, None, name="z")
    last = (bs - 1) * row_stride
    if z.dim() != 2 or z.shape[1] < dims[0] or z.shape[0] <= last:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [> {last}, >= {dims[0]}]")
    _need(batch_idx, (bs,), torch.int32, "batch_idx")
    _need(label_table, None, torch.int32, "label_table")
    if label_table.dim() != 1 or label_table.numel() < 1:
        raise ValueError(f"label_table: shape {tuple(label_table.shape)}, expected [N >= 1]")
    _need(class_weight, (dims[-1],), name="class_weight")
    n = mlp_param_count(dims)
    _need(params, (n,), name="params")
    _need(acc, (3,), name="acc")
    nbytes, ld_dlat = 0, 0
    if train:
        if (m is None) != (v is None) or (m is None and dw_out is None):
            raise ValueError("a train step takes m and v (Adam in place) or dw_out (the gradient only)")
        if m is not None:
            _need(m, (n,), name="m")
            _need(v, (n,), name="v")
        _need(step, (1,), torch.int32, "step")
        _need(dlat, None, name="dlat")
        if dlat.dim() != 2 or dlat.shape[1] < dims[0] or dlat.shape[0] <= last:
            raise ValueError(f"dlat: shape {tuple(dlat.shape)}, expected [> {last}, >= {dims[0]}]")
        ld_dlat = int(dlat.shape[1])
        workspace, nbytes = _conv_ws(workspace, z.device, mlp_workspace(dims, bs))
        if dw_out is not None:
            _need(dw_out, (n,), name="dw_out")
    call("cfsd_mlp_head_step", ptr(z), int(z.shape[1]), row_stride, ptr(batch_idx), ptr(label_table),
         int(label_table.numel()), ptr(class_weight), ptr(params), ptr(m) if train else None,
         ptr(v) if train else None, ptr(step) if train else None, ptr(acc), ptr(workspace) if train else None,
         ctypes.c_size_t(nbytes), ptr(dw_out) if train else None, ptr(dlat) if train else None, ld_dlat,
         float(w_cls), cdims, len(dims) - 1, bs, int(bool(train)), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), stream_ptr())


# ------------------------------------------------------------------ latent fitting
NN_TILE = _H["CFSD_NN_TILE"]  # reference points per chunk of cfsd_nn_points


def _points(t, name):
    _need(t, None, name=name)
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [B, N >= 1, 3]")
    return int(t.shape[0]), int(t.shape[1])


def _pair_batch(bq, br, what):
    bsz = max(bq, br)
    if bq not in (1, bsz) or br not in (1, bsz):
        raise ValueError(f"{what}: batch sizes {bq} and {br} must be equal or 1")
    return bsz


def nn_points(q, r, workspace=None):
    """Brute-force nearest neighbour (``cfsd_nn_points``): for every query of
    ``q`` ``[Bq, N, 3]`` the squared distance to, and the int32 index of, the
    nearest point of ``r`` ``[Br, P, 3]``.  ``Bq`` and ``Br`` are equal or 1; a
    batch of 1 is shared by every element of the other operand's batch (read
    in place, not expanded).  Equal distances resolve to the lowest index.
    Returns ``(dist2 [B, N] float32, idx [B, N] int32)``."""
    bq, n = _points(q, "q")
    br, p = _points(r, "r")
    if r.device != q.device:
        raise ValueError("q and r must be on one device")
    bsz = _pair_batch(bq, br, "nn_points")
    need = int(_abi.lib().cfsd_nn_points_workspace(bsz, n, p))
    nbytes = 0
    if need:
        workspace, nbytes = _conv_ws(workspace, q.device, need)
    else:
        workspace = None
    dist2 = torch.empty((bsz, n), dtype=torch.float32, device=q.device)
    idx = torch.empty((bsz, n), dtype=torch.int32, device=q.device)
    call("cfsd_nn_points", ptr(q), ptr(r), ptr(dist2), ptr(idx), ptr(workspace), nbytes, bsz, bq, br, n, p,
         stream_ptr())
    return dist2, idx


def chamfer_bwd(x, y, idx_xy, idx_yx, wx, wy):
    """Gradient of the two-sided Chamfer sum w.r.t. ``x`` (``cfsd_chamfer_bwd``):
    ``gx[b,i] = wx[b] 2(x_i - y[idx_xy[b,i]]) + wy[b] sum_{j: idx_yx[b,j]=i} 2(x_i - y_j)``.
    The targets of each generated point are grouped on the device (stable
    sort of ``idx_yx`` + segment offsets) and summed in ascending ``j`` by the
    kernel: deterministic, no atomics."""
    bsz, n = _points(x, "x")
    by, p = _points(y, "y")
    if by not in (1, bsz):
        raise ValueError(f"chamfer_bwd: y batch {by} must be 1 or {bsz}")
    _need(idx_xy, (bsz, n), torch.int32, "idx_xy")
    _need(idx_yx, (bsz, p), torch.int32, "idx_yx")
    _need(wx, (bsz,), name="wx")
    _need(wy, (bsz,), name="wy")
    keys, order = torch.sort(idx_yx, dim=1, stable=True)
    bounds = torch.arange(n + 1, dtype=torch.int32, device=x.device).expand(bsz, n + 1).contiguous()
    seg_ptr = torch.searchsorted(keys, bounds, out_int32=True).contiguous()
    seg_j = order.to(torch.int32).contiguous()
    gx = torch.empty_like(x)
    call("cfsd_chamfer_bwd", ptr(x), ptr(y), ptr(idx_xy), ptr(seg_ptr), ptr(seg_j), ptr(wx), ptr(wy), ptr(gx),
         bsz, by, n, p, stream_ptr())
    return gx


NN_GRID_MAX = _H["CFSD_NN_GRID_MAX"]  # most cells per axis of a PointGrid
# Points per cell the default cell count aims at, counted as P / g^2: the point sets of a fit are SURFACES, which
# occupy about g^2 of the g^3 cells.  Chosen by the sweep of tools/bench_fit_grid.py (profiles/fit_grid_sweep.json,
# DESIGN 8.2): the fastest of 1, 2, 4, 8, 16, 32 at every scan size.
NN_GRID_POINTS_PER_CELL = 32.0


def default_grid_cells(p):
    """The ``cells=None`` rule of :class:`PointGrid`: ``(g, g, g)`` with ``g =
    round(sqrt(P / NN_GRID_POINTS_PER_CELL))`` held to ``1 .. NN_GRID_MAX`` -- a
    function of the point COUNT alone, so choosing it reads nothing back."""
    g = int(min(max(round((int(p) / NN_GRID_POINTS_PER_CELL) ** 0.5), 1), NN_GRID_MAX))
    return (g, g, g)


def _grid_cells(cells, p):
    if cells is None:
        return default_grid_cells(p)
    try:
        cells = tuple(cells)
        ok = len(cells) == 3 and all(isinstance(g, int) and not isinstance(g, bool) for g in cells)
    except TypeError:
        ok = False
    if not ok or not all(1 <= g <= NN_GRID_MAX for g in cells):
        raise ValueError(f"PointGrid: cells={cells!r}, expected None or three integers in 1..{NN_GRID_MAX}")
    return cells


class PointGrid:
    """A point set ``[B, P, 3]`` (or ``[P, 3]``) with its uniform grid
    (``cfsd_nn_grid_build``) as the reference side of :func:`nn_points_grid`: a
    CONSTANT set is built once and searched many times, as
    :class:`SurfaceMesh` is for the surface term.  ``cells`` ``(gx, gy, gz)``,
    each in ``1 .. NN_GRID_MAX``, or None for :func:`default_grid_cells`.
    Every batch element has its own grid over its own bounding box; the box
    is computed on the device and never read back.

    A single set (``B = 1``) also holds ``queries`` ``[1, P, 3]``, its points
    in Morton order, and ``perm`` (``queries[0, i] = points[0, perm[i]]``),
    for searches FROM the set: a wave's 64 queries should be neighbours in
    space and a scan's vertex order is arbitrary (``queries=False`` skips
    them)."""

    def __init__(self, points, cells=None, queries=True):
        if not isinstance(points, torch.Tensor):
            raise ValueError("PointGrid: points must be a device float32 tensor [B, P, 3] or [P, 3]")
        cells = _grid_cells(cells, points.shape[-2] if points.dim() >= 2 else 1)
        points = points.detach()
        if points.dim() == 2:
            points = points[None]
        points = points.contiguous()
        self.batch, self.p = _points(points, "points")
        self.points, self.cells = points, cells
        gx, gy, gz = cells
        need = int(_abi.lib().cfsd_nn_grid_build_workspace(self.batch, self.p, gx, gy, gz))
        if need <= 0:
            raise ValueError(f"PointGrid: {self.batch} x {self.p} points in {cells} cells exceed 32-bit indices")
        self.workspace = torch.empty(need // 4, dtype=torch.int32, device=points.device)
        self.nbytes = ctypes.c_size_t(need)
        n = self.batch * self.p
        ids = self.workspace[need // 4 - (n + 3) // 4 * 4:][:n].view(self.batch, self.p)  # the buffer's last section
        self._build(_H["CFSD_NN_GRID_CELLS"], None, None)
        keys, order = torch.sort(ids, dim=1, stable=True)
        self._build(_H["CFSD_NN_GRID_GROUP"], keys.contiguous(), order.contiguous())
        self.queries = self.perm = None
        if queries and self.batch == 1:
            order = _morton_order(points[0])
            self.queries = points.index_select(1, order).contiguous()
            self.perm = order.to(torch.int32)

    def _build(self, stage, keys, order):
        gx, gy, gz = self.cells
        call("cfsd_nn_grid_build", ptr(self.points), ptr(self.workspace), self.nbytes, stage, ptr(keys), ptr(order),
             self.batch, self.p, gx, gy, gz, stream_ptr())


def nn_points_grid(q, grid, return_stats=False):
    """:func:`nn_points` through a uniform grid (``cfsd_nn_points_grid``):
    ``q`` ``[Bq, N, 3]`` against ``grid``, a :class:`PointGrid` over ``[Br, P,
    3]``; ``Bq`` and ``Br`` equal or 1.  Exact: ``(dist2, idx)`` are bit for
    bit those of ``nn_points(q, grid.points)``, equal distances resolved to
    the lowest index, in the caller's order.  ``q`` may itself be a single-set
    :class:`PointGrid`: its points then query in Morton order and the results
    are written back in the set's own order.  ``return_stats`` appends the
    int32 ``[B, N]`` count of points evaluated per query."""
    if not isinstance(grid, PointGrid):
        raise ValueError("nn_points_grid: grid must be a PointGrid")
    perm = None
    if isinstance(q, PointGrid):
        q, perm = (q.queries, q.perm) if q.perm is not None else (q.points, None)
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise ValueError("nn_points_grid: q must be a [B, N, 3] tensor or a PointGrid")
    bsz = _pair_batch(int(q.shape[0]), grid.batch, "nn_points_grid")
    bq, n = _points(q, "q")
    if grid.points.device != q.device:
        raise ValueError("q and the grid must be on one device")
    dist2 = torch.empty((bsz, n), dtype=torch.float32, device=q.device)
    idx = torch.empty((bsz, n), dtype=torch.int32, device=q.device)
    count = torch.empty((bsz, n), dtype=torch.int32, device=q.device) if return_stats else None
    gx, gy, gz = grid.cells
    call("cfsd_nn_points_grid", ptr(q), ptr(grid.workspace), grid.nbytes, ptr(perm), ptr(dist2), ptr(idx), ptr(count),
         bsz, bq, grid.batch, n, grid.p, gx, gy, gz, stream_ptr())
    return (dist2, idx, count) if return_stats else (dist2, idx)


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, point_mean, y_grid=None):
        if y_grid is None:
            d_xy, i_xy = nn_points(x, y)
            d_yx, i_yx = nn_points(y, x)
        else:  # the same distances and indices, bit for bit, through the grids
            d_xy, i_xy = nn_points_grid(x, y_grid)
            d_yx, i_yx = nn_points_grid(y_grid if y_grid.perm is not None else y, PointGrid(x, queries=False))
        ctx.save_for_backward(x, y, i_xy, i_yx)
        ctx.point_mean = point_mean
        cx, cy = d_xy.sum(1), d_yx.sum(1)
        if point_mean:
            cx, cy = cx / x.shape[1], cy / y.shape[1]
        return cx + cy  # [B]

    @staticmethod
    def backward(ctx, g):
        x, y, i_xy, i_yx = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        wx = g / x.shape[1] if ctx.point_mean else g
        wy = g / y.shape[1] if ctx.point_mean else g.clone()
        return chamfer_bwd(x, y, i_xy, i_yx, wx.contiguous(), wy.contiguous()), None, None, None


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction="mean", norm=2, search="brute"):
    """The subset of ``pytorch3d.loss.chamfer_distance`` the reference's
    fitting uses (``test.py:404-405, 427-429``), on libcfsd.

    ``x`` ``[B, N, 3]`` generated points (may require grad), ``y`` ``[B or 1,
    P, 3]`` target points (constant).  Per batch element: the mean (or sum)
    over ``x`` of the squared distance to the nearest ``y``, plus the same from
    ``y`` to ``x``; then ``batch_reduction`` ``"mean"``, ``"sum"`` or ``None``
    (``[B]``).  Lengths, normals, weights and other norms raise
    ``ValueError``.  Returns ``(loss, None)`` like pytorch3d (no normals
    term).

    ``search``: ``"brute"`` (the default) walks every pair (``nn_points``);
    ``"grid"`` runs both directions through uniform grids
    (:func:`nn_points_grid`) -- for dense targets.  ``y`` may then be a
    :class:`PointGrid`, built once and reused over many calls; the grid over
    ``x`` is built per call.  Loss and gradient are bit-identical to
    ``"brute"``: the same distances summed in the same order, the same indices
    into the same ``chamfer_bwd``.  Any other value raises ``ValueError``."""
    if search not in ("brute", "grid"):
        raise ValueError(f'chamfer_distance: search={search!r}, expected "brute" or "grid"')
    y_grid = None
    if isinstance(y, PointGrid):
        if search != "grid":
            raise ValueError('chamfer_distance: a PointGrid target needs search="grid"')
        y_grid, y = y, y.points
    if x_lengths is not None or y_lengths is not None:
        raise ValueError("chamfer_distance: x_lengths / y_lengths are not supported (dense point sets only)")
    if x_normals is not None or y_normals is not None:
        raise ValueError("chamfer_distance: normals are not supported")
    if weights is not None:
        raise ValueError("chamfer_distance: weights are not supported")
    if norm != 2:
        raise ValueError("chamfer_distance: only norm=2 (squared L2) is supported")
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if y.requires_grad:
        raise ValueError("chamfer_distance: the target y is a constant (no gradient is computed for it)")
    x, y = x.contiguous(), y.contiguous()
    bsz, _ = _points(x, "x")
    by, _ = _points(y, "y")
    if by not in (1, bsz):
        raise ValueError(f"chamfer_distance: y batch {by} must be 1 or {bsz}")
    if search == "grid" and y_grid is None:
        y_grid = PointGrid(y)
    per_batch = _ChamferFn.apply(x, y, point_reduction == "mean", y_grid)
    if batch_reduction == "mean":
        return per_batch.sum() / bsz, None
    if batch_reduction == "sum":
        return per_batch.sum(), None
    return per_batch, None


# ------------------------------------------------------------------ surface fitting
PF_GROUP = _H["CFSD_PF_GROUP"]  # faces per group sphere of cfsd_point_face
PF_CULL, PF_PREPARED = _H["CFSD_PF_CULL"], _H["CFSD_PF_PREPARED"]  # its flags
PF_WAVE = 64       # queries per workgroup of cfsd_point_face: one row of its stats


class FaceTable:
    """A validated ``[F, 3]`` int32 face tensor of a mesh with ``n_verts``
    vertices, and what seeds the culled search: ``ref_idx`` ``[R]`` the
    vertices some face references (ascending) and ``vert_face`` ``[R]`` int32
    the lowest face at each.  Built by :func:`face_table`."""

    def __init__(self, faces, n_verts):
        _need(faces, None, torch.int32, "faces")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError(f"faces: shape {tuple(faces.shape)}, expected [F >= 1, 3]")
        lo, hi = torch.aminmax(faces)
        lo, hi = int(lo), int(hi)  # the one host read, once per face tensor
        if lo < 0 or hi >= n_verts:
            raise ValueError(f"faces: indices span [{lo}, {hi}], outside [0, {n_verts})")
        nf = int(faces.shape[0])
        fid = torch.arange(nf, device=faces.device).repeat_interleave(3)
        first = torch.full((n_verts,), nf, dtype=torch.long, device=faces.device)
        first.scatter_reduce_(0, faces.reshape(-1).long(), fid, "amin")
        self.faces, self.n_verts, self.n_faces = faces, int(n_verts), nf
        self.ref_idx = torch.nonzero(first < nf).reshape(-1)
        self.vert_face = first[self.ref_idx].to(torch.int32)


_FACE_TABLES = {}  # (data_ptr, version, F, n_verts, device) -> FaceTable (holds the tensor: the key stays its own)


def face_table(faces, n_verts):
    """The :class:`FaceTable` of ``faces``.  Host tensors, wrong ranks or
    dtypes and indices outside ``[0, n_verts)`` raise ``ValueError``; the
    index check reads the device once per face tensor (the few most recent
    tables are kept, keyed by the tensor's storage and version)."""
    if isinstance(faces, FaceTable):
        if faces.n_verts != n_verts:
            raise ValueError(f"faces: table built for {faces.n_verts} vertices, mesh has {n_verts}")
        return faces
    if not isinstance(faces, torch.Tensor):
        raise ValueError("faces must be a device int32 tensor [F, 3]")
    key = (faces.data_ptr(), faces._version, tuple(faces.shape), faces.dtype, int(n_verts), str(faces.device))
    tab = _FACE_TABLES.pop(key, None)
    if tab is None:
        tab = FaceTable(faces, int(n_verts))
    _FACE_TABLES[key] = tab  # most recent last
    while len(_FACE_TABLES) > 8:
        _FACE_TABLES.pop(next(iter(_FACE_TABLES)))
    return tab


def _morton_order(p):
    """Permutation of the points ``p`` ``[P, 3]`` along a 30-bit Morton curve
    of their bounding box (device only, no host read): consecutive points are
    neighbours in space, whatever order the file listed them in."""
    lo, hi = p.min(0).values, p.max(0).values
    q = ((p - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).long().clamp_(0, 1023)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    return torch.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2), stable=True)


class SurfaceMesh:
    """A CONSTANT mesh as the target of repeated searches: ``verts`` ``[1, V,
    3]``, its :class:`FaceTable`, its referenced vertices and the workspace
    that keeps the per-face records of ``cfsd_point_face`` after the first
    search, so that later ones skip the pre-launch.  ``queries`` ``[1, V, 3]``
    are the same vertices in Morton order, for searches FROM the mesh: a wave
    of ``cfsd_point_face`` culls for its 64 consecutive queries together, and
    a scan's vertex order is arbitrary."""

    def __init__(self, verts, faces):
        verts = verts.detach()
        if verts.dim() == 2:
            verts = verts[None]
        verts = verts.contiguous()
        bv, nv = _points(verts, "verts")
        if bv != 1:
            raise ValueError(f"SurfaceMesh: one mesh expected, got a batch of {bv}")
        self.verts, self.table = verts, face_table(faces, nv)
        self.ref = verts.index_select(1, self.table.ref_idx).contiguous()
        need = int(_abi.lib().cfsd_point_face_workspace(1, self.table.n_faces))
        self.workspace = torch.empty(need // 4, dtype=torch.float32, device=verts.device)
        self.prepared = False
        self.queries = verts.index_select(1, _morton_order(verts[0])).contiguous()


def point_face_distance(points, verts, faces=None, cull=True, return_stats=False):
    """Nearest point of a triangle mesh (``cfsd_point_face``): for every point
    of ``points`` ``[Bp, N, 3]`` the squared distance to the closed triangles
    ``faces`` ``[F, 3]`` (int32, shared by the batch) of ``verts`` ``[Bv, V,
    3]``, the int32 index of the nearest face (equal distances: the lowest)
    and the barycentric weights of the nearest point on it.  ``Bp`` and ``Bv``
    are equal or 1.  ``verts`` may be a :class:`SurfaceMesh` (then ``faces`` is
    not given).

    ``cull=True`` seeds every point's bound with a face at its nearest
    referenced vertex (``nn_points`` over the vertices that a face uses) and
    skips groups and faces whose bounding sphere is out of reach;
    ``cull=False`` evaluates every pair.  The results are bit-identical.
    Returns ``(dist2 [B, N] float32, face_idx [B, N] int32, bary [B, N, 3]
    float32)``, with ``return_stats`` also ``[B * ceil(N / 64), 2]`` int32:
    per wave of 64 points the groups entered and the faces evaluated."""
    mesh = verts if isinstance(verts, SurfaceMesh) else None
    if mesh is not None:
        if faces is not None:
            raise ValueError("point_face_distance: a SurfaceMesh carries its own faces")
        verts, tab = mesh.verts, mesh.table
    bp, n = _points(points, "points")
    bv, nv = _points(verts, "verts")
    if verts.device != points.device:
        raise ValueError("points and verts must be on one device")
    if mesh is None:
        tab = face_table(faces, nv)
    bsz = _pair_batch(bp, bv, "point_face_distance")
    dev, nf = points.device, tab.n_faces
    if mesh is not None:
        workspace = mesh.workspace
    else:
        workspace = torch.empty(int(_abi.lib().cfsd_point_face_workspace(bv, nf)) // 4, dtype=torch.float32,
                                device=dev)
    flags, seed = 0, None
    if cull:
        flags |= PF_CULL
        ref = mesh.ref if mesh is not None else verts.index_select(1, tab.ref_idx).contiguous()
        seed = tab.vert_face[nn_points(points, ref)[1].long()].contiguous()
    if mesh is not None and mesh.prepared:
        flags |= PF_PREPARED
    dist2 = torch.empty((bsz, n), dtype=torch.float32, device=dev)
    face_idx = torch.empty((bsz, n), dtype=torch.int32, device=dev)
    bary = torch.empty((bsz, n, 3), dtype=torch.float32, device=dev)
    stats = None
    if return_stats:
        stats = torch.empty((bsz * ((n + PF_WAVE - 1) // PF_WAVE), 2), dtype=torch.int32, device=dev)
    call("cfsd_point_face", ptr(points), ptr(verts), ptr(tab.faces), ptr(seed), ptr(dist2), ptr(face_idx),
         ptr(bary), ptr(stats), ptr(workspace), workspace.numel() * 4, bsz, bp, bv, n, nv, nf, flags, stream_ptr())
    if mesh is not None:
        mesh.prepared = True
    return (dist2, face_idx, bary, stats) if return_stats else (dist2, face_idx, bary)


def point_face_bwd(points, verts, faces, face_idx, bary, g, want_verts):
    """Gradient of ``sum g * dist2`` through fixed faces and weights
    (``cfsd_point_face_bwd``): ``gp [B, N, 3] = g 2 (p - c)`` and, with
    ``want_verts``, ``gv [B, V, 3]``, each vertex's ``-gp * weight``
    contributions grouped on the device (stable sort of the winning faces'
    corners + run offsets) and summed in ascending order by one thread:
    deterministic, no atomics.  Returns ``(gp, gv or None)`` at the full batch."""
    bp, n = _points(points, "points")
    bv, nv = _points(verts, "verts")
    bsz = _pair_batch(bp, bv, "point_face_bwd")
    tab = face_table(faces, nv)
    _need(face_idx, (bsz, n), torch.int32, "face_idx")
    _need(bary, (bsz, n, 3), name="bary")
    _need(g, (bsz, n), name="g")
    gp = torch.empty((bsz, n, 3), dtype=torch.float32, device=points.device)
    seg_ptr = seg_e = gv = None
    if want_verts:
        corners = tab.faces[face_idx.long()].reshape(bsz, 3 * n)  # vertex of pair i * 3 + k
        keys, order = torch.sort(corners, dim=1, stable=True)
        bounds = torch.arange(nv + 1, dtype=torch.int32, device=points.device).expand(bsz, nv + 1).contiguous()
        seg_ptr = torch.searchsorted(keys, bounds, out_int32=True).contiguous()
        seg_e = order.to(torch.int32).contiguous()
        gv = torch.empty((bsz, nv, 3), dtype=torch.float32, device=points.device)
    call("cfsd_point_face_bwd", ptr(points), ptr(verts), ptr(tab.faces), ptr(face_idx), ptr(bary), ptr(g), ptr(gp),
         ptr(seg_ptr), ptr(seg_e), ptr(gv), bsz, bp, bv, n, nv, tab.n_faces, stream_ptr())
    return gp, gv


class _PointMeshFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, verts, target):
        """``target``: the mesh's SurfaceMesh (then ``verts`` is its tensor) or FaceTable."""
        mesh = target if isinstance(target, SurfaceMesh) else None
        dist2, face_idx, bary = point_face_distance(points, mesh if mesh is not None else verts,
                                                    None if mesh is not None else target)
        ctx.save_for_backward(points, verts, face_idx, bary)
        ctx.table = target.table if mesh is not None else target
        ctx.mark_non_differentiable(face_idx, bary)
        return dist2, face_idx, bary

    @staticmethod
    def backward(ctx, g, _gi, _gb):
        points, verts, face_idx, bary = ctx.saved_tensors
        want_p, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gp, gv = point_face_bwd(points, verts, ctx.table, face_idx, bary, g.contiguous().to(torch.float32), want_v)
        if want_p and points.shape[0] != gp.shape[0]:
            gp = gp.sum(0, keepdim=True)
        if want_v and verts.shape[0] != gv.shape[0]:
            gv = gv.sum(0, keepdim=True)
        return (gp if want_p else None), (gv if want_v else None), None


def _mesh_operands(verts, faces, what):
    """(verts tensor, SurfaceMesh or FaceTable) of a mesh given either way."""
    if isinstance(verts, SurfaceMesh):
        if faces is not None:
            raise ValueError(f"{what}: a SurfaceMesh carries its own faces")
        return verts.verts, verts
    _, nv = _points(verts, "verts")
    return verts, face_table(faces, nv)


def point_mesh_distance(points, verts, faces=None, return_faces=False):
    """Squared distance of every point to the surface of a mesh, ``[B, N]``,
    differentiable in ``points`` and in ``verts`` (whichever requires grad)
    through the nearest faces and weights found (``point_face_distance``'s
    culled search; the backward is ``cfsd_point_face_bwd``).  ``verts`` may be
    a :class:`SurfaceMesh` (a constant).  With ``return_faces`` also the face
    indices and weights."""
    _points(points, "points")
    verts, target = _mesh_operands(verts, faces, "point_mesh_distance")
    if verts.device != points.device:
        raise ValueError("points and verts must be on one device")
    dist2, face_idx, bary = _PointMeshFn.apply(points, verts, target)
    return (dist2, face_idx, bary) if return_faces else dist2


def surface_distance(gen_verts, gen_faces, scan_verts, scan_faces=None, batch_reduction="mean"):
    """The surface term of the fit: per batch element the mean over the
    generated vertices ``gen_verts`` ``[B, V, 3]`` of the squared distance to
    the scan's surface, plus the mean over the scan's vertices of the squared
    distance to the generated surface (``gen_faces`` ``[F, 3]``).  The scan is
    a constant: ``scan_verts`` ``[1, P, 3]`` with ``scan_faces`` ``[Fs, 3]``,
    or a :class:`SurfaceMesh` holding both (its per-face records, referenced
    vertices and query order are then computed once, not per call).
    ``batch_reduction`` ``"mean"``, ``"sum"`` or ``None``
    (``[B]``), as in :func:`chamfer_distance`."""
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if isinstance(scan_verts, SurfaceMesh):
        if scan_faces is not None:
            raise ValueError("surface_distance: a SurfaceMesh carries its own faces")
        mesh = scan_verts
    else:
        if scan_verts.requires_grad:
            raise ValueError("surface_distance: the scan is a constant (no gradient is computed for it)")
        mesh = SurfaceMesh(scan_verts, scan_faces)
    gen_verts = gen_verts.contiguous()
    bsz, _ = _points(gen_verts, "gen_verts")
    to_scan = point_mesh_distance(gen_verts, mesh)
    to_gen = point_mesh_distance(mesh.queries, gen_verts, gen_faces)
    per_batch = to_scan.mean(1) + to_gen.mean(1)
    if batch_reduction == "mean":
        return per_batch.sum() / bsz
    if batch_reduction == "sum":
        return per_batch.sum()
    return per_batch


# ------------------------------------------------------------------ rendering
RN_GROUP = _H["CFSD_RN_GROUP"]        # faces per group box of cfsd_rasterize
RN_MAX_SIZE = _H["CFSD_RN_MAX_SIZE"]  # largest image side


class RenderFaces:
    """A face tensor prepared for rendering: its :class:`FaceTable` and the
    vertex -> faces runs of the normals (``vf_ptr`` ``[V + 1]``, ``vf_idx``
    ``[3 F]`` int32: the face of every corner grouped by vertex, ascending, so
    a vertex's normal is summed in one fixed order).  Built by
    :func:`render_faces`."""

    def __init__(self, table):
        faces, nv = table.faces, table.n_verts
        keys, order = torch.sort(faces.reshape(-1), stable=True)  # corner e = f * 3 + k: ascending f within a vertex
        bounds = torch.arange(nv + 1, dtype=torch.int32, device=faces.device)
        self.table = table
        self.faces, self.n_verts, self.n_faces = faces, nv, table.n_faces
        self.vf_ptr = torch.searchsorted(keys, bounds, out_int32=True).contiguous()
        self.vf_idx = (order // 3).to(torch.int32).contiguous()


_RENDER_FACES = {}  # id(FaceTable) -> RenderFaces (holds the table: the key stays its own)


def render_faces(faces, n_verts):
    """The :class:`RenderFaces` of ``faces`` (validated and cached the way
    :func:`face_table` caches its tables)."""
    if isinstance(faces, RenderFaces):
        if faces.n_verts != n_verts:
            raise ValueError(f"faces: prepared for {faces.n_verts} vertices, mesh has {n_verts}")
        return faces
    tab = face_table(faces, n_verts)
    rf = _RENDER_FACES.pop(id(tab), None)
    if rf is None or rf.table is not tab:
        rf = RenderFaces(tab)
    _RENDER_FACES[id(tab)] = rf
    while len(_RENDER_FACES) > 8:
        _RENDER_FACES.pop(next(iter(_RENDER_FACES)))
    return rf


def _image_size(image_size):
    s = int(image_size)
    if s != image_size or s < 1 or s > RN_MAX_SIZE:
        raise ValueError(f"image_size {image_size!r}: an integer in [1, {RN_MAX_SIZE}] expected")
    return s


def _rgb(value, name="background"):
    """A colour given as one number or three."""
    try:
        v = [float(value)] * 3
    except TypeError:
        v = [float(c) for c in value]
    if len(v) != 3:
        raise ValueError(f"{name}: one value or three expected")
    return v


def _vertex_colors(colors, bsz, nv, device):
    _need(colors, None, name="colors")
    if colors.dim() != 3 or colors.shape[0] not in (1, bsz) or tuple(colors.shape[1:]) != (nv, 3):
        raise ValueError(f"colors: shape {tuple(colors.shape)}, expected [{bsz} or 1, {nv}, 3]")
    if colors.device != device:
        raise ValueError("colors must be on the meshes' device")
    return int(colors.shape[0])


def vertex_normals(verts, faces):
    """Area-weighted vertex normals ``[B, V, 3]`` of ``verts`` ``[B, V, 3]``
    with ``faces`` ``[F, 3]`` (int32, shared by the batch): the normalised sum
    of the un-normalised face normals at each vertex, zero for a vertex no
    face uses (``cfsd_vertex_normals``)."""
    bsz, nv = _points(verts, "verts")
    rf = render_faces(faces, nv)
    out = torch.empty_like(verts)
    call("cfsd_vertex_normals", ptr(verts), ptr(rf.faces), ptr(rf.vf_ptr), ptr(rf.vf_idx), ptr(out), bsz, nv,
         rf.n_faces, stream_ptr())
    return out


def project_vertices(verts, camera, faces=None, tex=None, light=(0.0, 0.0, 3.0), ambient=0.5, diffuse=1.0,
                     specular=0.2, shininess=0.5, tex_value=0.5, shade=False):
    """View transform and projection of ``verts`` ``[B, V, 3]`` by ``camera``
    (a :class:`rendering.Camera`): ``(ndc_xy [B, V, 2], view_z [B, V])`` and,
    with ``shade``, the Gouraud vertex colours ``[B, V, 3]`` (else None):
    ``(ambient + diffuse max(n.L, 0)) tex + specular spec`` with ``tex`` ``[B
    or 1, V, 3]`` or the constant ``tex_value`` (``cfsd_render_vertices``)."""
    bsz, nv = _points(verts, "verts")
    dev = verts.device
    ndc = torch.empty((bsz, nv, 2), dtype=torch.float32, device=dev)
    vz = torch.empty((bsz, nv), dtype=torch.float32, device=dev)
    colors = fp = vp = vi = None
    bt, nf = 1, 1
    if shade:
        rf = render_faces(faces, nv)
        fp, vp, vi, nf = rf.faces, rf.vf_ptr, rf.vf_idx, rf.n_faces
        if tex is not None:
            bt = _vertex_colors(tex, bsz, nv, dev)
        colors = torch.empty((bsz, nv, 3), dtype=torch.float32, device=dev)
    lx, ly, lz = (float(c) for c in light)
    call("cfsd_render_vertices", ptr(verts), ptr(camera.tensor(dev)), ptr(fp), ptr(vp), ptr(vi), ptr(tex), ptr(ndc),
         ptr(vz), ptr(colors), bsz, bt, nv, nf, lx, ly, lz, float(ambient), float(diffuse), float(specular),
         float(shininess), float(tex_value), stream_ptr())
    return ndc, vz, colors


def rasterize_ndc(ndc_xy, view_z, faces, image_size, znear=1.0, colors=None, background=0.0):
    """The raster stage on projected vertices (``cfsd_rasterize``): ``ndc_xy``
    ``[B, V, 2]``, ``view_z`` ``[B, V]``, ``faces`` ``[F, 3]`` int32 shared by
    the batch.  Returns ``(pix_to_face [B, S, S] int32, zbuf [B, S, S], bary
    [B, S, S, 3])`` with -1 on background pixels; with ``colors`` ``[B or 1,
    V, 3]`` also the interpolated image ``[B, 3, S, S]`` over ``background``
    (written by the same launch).  A face with a vertex at ``view_z <= znear``
    is dropped."""
    _need(ndc_xy, None, name="ndc_xy")
    if ndc_xy.dim() != 3 or ndc_xy.shape[-1] != 2 or ndc_xy.shape[0] < 1 or ndc_xy.shape[1] < 1:
        raise ValueError(f"ndc_xy: shape {tuple(ndc_xy.shape)}, expected [B, V >= 1, 2]")
    bsz, nv = int(ndc_xy.shape[0]), int(ndc_xy.shape[1])
    _need(view_z, (bsz, nv), name="view_z")
    if view_z.device != ndc_xy.device:
        raise ValueError("ndc_xy and view_z must be on one device")
    tab = face_table(faces.table if isinstance(faces, RenderFaces) else faces, nv)
    size, dev = _image_size(image_size), ndc_xy.device
    bc, image = 1, None
    if colors is not None:
        bc = _vertex_colors(colors, bsz, nv, dev)
        image = torch.empty((bsz, 3, size, size), dtype=torch.float32, device=dev)
    bg = _rgb(background)
    if bsz * size * size * 3 >= 2 ** 31:
        raise ValueError("rasterize: batch x pixels x 3 must stay below 2^31")
    pix_to_face = torch.empty((bsz, size, size), dtype=torch.int32, device=dev)
    zbuf = torch.empty((bsz, size, size), dtype=torch.float32, device=dev)
    bary = torch.empty((bsz, size, size, 3), dtype=torch.float32, device=dev)
    need = int(_abi.lib().cfsd_raster_workspace(bsz, tab.n_faces))
    workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    call("cfsd_rasterize", ptr(ndc_xy), ptr(view_z), ptr(tab.faces), ptr(colors), ptr(pix_to_face), ptr(zbuf),
         ptr(bary), ptr(image), ptr(workspace), need, bsz, bc, nv, tab.n_faces, size, float(znear), bg[0], bg[1],
         bg[2], stream_ptr())
    return (pix_to_face, zbuf, bary) if colors is None else (pix_to_face, zbuf, bary, image)


def rasterize_meshes(verts, faces, camera, image_size):
    """``verts`` ``[B, V, 3]`` seen by ``camera`` (a
    :class:`rendering.Camera`): ``(pix_to_face, zbuf, bary)`` as
    :func:`rasterize_ndc` returns them."""
    _points(verts, "verts")
    _image_size(image_size)
    ndc, vz, _ = project_vertices(verts, camera)
    return rasterize_ndc(ndc, vz, faces, image_size, znear=camera.znear)


def interpolate_vertex_colors(pix_to_face, bary, faces, colors, background=0.0):
    """The image ``[B, 3, S, S]`` of a finished raster stage: per covered
    pixel the ``bary`` mix of the winning face's vertex colours (``colors``
    ``[B or 1, V, 3]``), ``background`` elsewhere (``cfsd_interpolate_colors``)."""
    _need(pix_to_face, None, torch.int32, "pix_to_face")
    if pix_to_face.dim() != 3 or pix_to_face.shape[1] != pix_to_face.shape[2] or pix_to_face.shape[0] < 1:
        raise ValueError(f"pix_to_face: shape {tuple(pix_to_face.shape)}, expected [B, S, S]")
    bsz, size = int(pix_to_face.shape[0]), _image_size(pix_to_face.shape[1])
    _need(bary, (bsz, size, size, 3), name="bary")
    _need(colors, None, name="colors")
    if colors.dim() != 3:
        raise ValueError(f"colors: shape {tuple(colors.shape)}, expected [B or 1, V, 3]")
    nv, dev = int(colors.shape[1]), pix_to_face.device
    bc = _vertex_colors(colors, bsz, nv, dev)
    tab = face_table(faces.table if isinstance(faces, RenderFaces) else faces, nv)
    bg = _rgb(background)
    image = torch.empty((bsz, 3, size, size), dtype=torch.float32, device=dev)
    call("cfsd_interpolate_colors", ptr(pix_to_face), ptr(bary), ptr(tab.faces), ptr(colors), ptr(image), bsz, bc, nv,
         tab.n_faces, size, bg[0], bg[1], bg[2], stream_ptr())
    return image


# ------------------------------------------------------------------ bf16 path
# Mixed-precision entry points (include/cfsd.h "bf16 path"): activations /
# gradients are float32 or bfloat16 tensors, weights are the fp32 master view
# and its bf16 shadow view.
def cast(src, out):
    """fp32 <-> bf16 storage conversion (round to nearest even)."""
    _needx(src, None, "src")
    _needx(out, tuple(src.shape), "out")
    call("cfsd_cast", ptr(src), _dt(src), ptr(out), _dt(out), ctypes.c_size_t(src.numel()), stream_ptr())
    return out


def spiral_conv_fwd_x(x, idx, w, w_bf16, b, act, out):
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), w.shape[0]
    _needl(x, None, "x")
    _need(w, (cout, seq * cin), name="w")
    if w_bf16 is not None:
        _need(w_bf16, (cout, seq * cin), torch.bfloat16, "w_bf16")
    if b is not None:
        _need(b, (cout,), name="bias")
    _needl(out, (bsz, rows, cout), "out")
    call("cfsd_spiral_conv_fwd_x", ptr(x), _st(x), ptr(idx), ptr(w), ptr(w_bf16), ptr(b), ptr(out),
         _st(out), bsz, vsrc, rows, seq, cin, cout, act, stream_ptr())
    return out


def spiral_conv_bwd_data_x(dpre, inv, w_bf16, vsrc, elu_y=None, out=None):
    bsz, rows, cout = dpre.shape
    seq = (inv[0].numel() - 1) // vsrc
    cin = w_bf16.shape[1] // seq
    _needl(dpre, None, "dpre")
    inv_ptr, inv_row, inv_head = _need_inv(inv, vsrc, rows, seq)
    _need(w_bf16, (cout, seq * cin), torch.bfloat16, "w_bf16")
    if out is None:
        out = torch.empty((bsz, vsrc, cin), dtype=torch.bfloat16, device=dpre.device)
    _needl(out, (bsz, vsrc, cin), "dx", torch.bfloat16)
    _need_like(out, "dx", (bsz, vsrc, cin), torch.bfloat16, elu_y=elu_y)
    call("cfsd_spiral_conv_bwd_data_x", ptr(dpre), _st(dpre), ptr(inv_ptr), ptr(inv_row), ptr(inv_head),
         ptr(w_bf16), ptr(elu_y), ptr(out), _st(out), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return out


def spiral_conv_bwd_data_flat(dpre, flat, w, vsrc, elu_y=None, out=None):
    """dx of a vertex-major layer through the flat inverse list
    (``topology.spiral_flat``), batch a multiple of 16.  ``w`` bf16 (the
    shadow; dx / elu_y bf16) or fp32 (dx, elu_y and dpre fp32: the fp32
    step's vertex-major kernel)."""
    bsz, rows, cout = dpre.shape
    seq = 9
    cin = w.shape[1] // seq
    dt = w.dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise ValueError(f"w must be fp32 or bf16, got {dt}")
    _needl(dpre, None, "dpre")
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, seq * cin), dt, "w")
    if out is None:
        out = vm_empty(bsz, vsrc, cin, dtype=dt, device=dpre.device)
    _needl(out, (bsz, vsrc, cin), "dx", dt)
    if dt == torch.float32 and dpre.dtype != torch.float32:
        raise ValueError("fp32 dx needs fp32 dpre")
    _need_like(out, "dx", (bsz, vsrc, cin), dt, elu_y=elu_y)
    call("cfsd_spiral_conv_bwd_data_flat", ptr(dpre), _st(dpre), ptr(table), width, ptr(w), ptr(elu_y),
         ptr(out), _st(out), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return out


def spiral_conv_bwd_weight_x_workspace(bsz, rows, seq, cin, cout, x_dtype=torch.bfloat16):
    """Workspace of :func:`spiral_conv_bwd_weight_x` (``x_dtype`` fp32: the
    fp32 kernels' slab geometry, as :func:`spiral_conv_bwd_weight_workspace`)."""
    if x_dtype == torch.float32:
        return spiral_conv_bwd_weight_workspace(bsz, rows, seq, cin, cout)
    return int(_abi.lib().cfsd_spiral_conv_bwd_weight_x_workspace(bsz, rows, seq, cin, cout))


def spiral_conv_bwd_weight_x(x, idx, dpre, dw, db, workspace):
    """dW/db of a bf16-path conv (x / dpre fp32 or bf16); ``dw is db is None``
    defers the reduction (returns a DeferredDw for dw_reduce_batch)."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _needl(x, None, "x")
    _needl(dpre, (bsz, rows, cout), "dpre")
    _need_dw_db(dw, db, cout, seq * cin)
    workspace, nbytes = _conv_ws(_need(workspace, None, name="workspace"), x.device,
                                 spiral_conv_bwd_weight_x_workspace(bsz, rows, seq, cin, cout, x.dtype))
    call("cfsd_spiral_conv_bwd_weight_x", ptr(x), _st(x), ptr(idx), ptr(dpre), _st(dpre), ptr(dw), ptr(db),
         ptr(workspace), ctypes.c_size_t(nbytes), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    # the code is the library's own routing decision for these operands
    code = _abi.lib().cfsd_spiral_conv_bwd_weight_x_slabs(_st(x), _st(dpre), bsz, cin, cout)
    return _deferred(dw, workspace, bsz, vsrc, rows, cin, cout, code)


def spiral_conv_bwd_flat_pair_workspace(bsz, rows, seq, cin, cout):
    return int(_abi.lib().cfsd_spiral_conv_bwd_flat_pair_workspace(bsz, rows, seq, cin, cout))


def spiral_conv_bwd_flat_pair(x, idx, dpre, flat, w, dw, db, dx, elu_y=None, workspace=None):
    """Both gradients of a full 32 -> 32 conv whose x, dpre, dx (and elu_y)
    are all vertex-major fp32 (the fp32 step's level-0/1 Deblocks) in ONE
    launch (``cfsd_spiral_conv_bwd_flat_pair``, ABI 4.10): the flat-list dx
    of :func:`spiral_conv_bwd_data_flat` and coarse-geometry dW slabs.
    ``dw is db is None`` defers the reduction (returns a DeferredDw)."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _need_vm(x, (bsz, vsrc, cin), "x", torch.float32)
    _need_vm(dpre, (bsz, rows, cout), "dpre", torch.float32)
    _need_vm(dx, (bsz, vsrc, cin), "dx", torch.float32)
    _need_like(dx, "dx", (bsz, vsrc, cin), torch.float32, elu_y=elu_y)
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, seq * cin), torch.float32, "w")
    _need_dw_db(dw, db, cout, seq * cin)
    need = spiral_conv_bwd_flat_pair_workspace(bsz, rows, seq, cin, cout)
    if need == 0:
        raise ValueError(f"no vertex-major pair for {cin} -> {cout} channels")
    ws, nb = _conv_ws(workspace, x.device, need)
    call("cfsd_spiral_conv_bwd_flat_pair", ptr(x), ptr(idx), ptr(dpre), ptr(table), width, ptr(w), ptr(elu_y),
         ptr(dx), ptr(dw), ptr(db), ptr(ws), ctypes.c_size_t(nb), bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return _deferred(dw, ws, bsz, vsrc, rows, cin, cout, DW_VM32)


def spiral_conv_bwd_flat_pair_bf16(x, idx, dpre, flat, w16, dx, elu_y=None, workspace=None):
    """:func:`spiral_conv_bwd_flat_pair` on the bf16 step's tensors (x, dpre,
    dx, elu_y bf16 vertex-major; ``w16`` the bf16 weight shadow), always
    deferred (``cfsd_spiral_conv_bwd_flat_pair_bf16``, ABI 4.11): the dx of
    :func:`spiral_conv_bwd_data_flat` and the slabs of
    :func:`spiral_conv_bwd_weight_x` in one launch; returns the DeferredDw."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _need_vm(x, (bsz, vsrc, cin), "x", torch.bfloat16)
    _need_vm(dpre, (bsz, rows, cout), "dpre", torch.bfloat16)
    _need_vm(dx, (bsz, vsrc, cin), "dx", torch.bfloat16)
    _need_like(dx, "dx", (bsz, vsrc, cin), torch.bfloat16, elu_y=elu_y)
    table, width = _need_flat(flat, vsrc)
    _need(w16, (cout, seq * cin), torch.bfloat16, "w16")
    workspace, nbytes = _conv_ws(_need(workspace, None, name="workspace"), x.device,
                                 spiral_conv_bwd_weight_x_workspace(bsz, rows, seq, cin, cout))
    call("cfsd_spiral_conv_bwd_flat_pair_bf16", ptr(x), ptr(idx), ptr(dpre), ptr(table), width, ptr(w16),
         ptr(elu_y), ptr(dx), ptr(workspace), ctypes.c_size_t(nbytes), bsz, vsrc, rows, seq, cin, cout,
         stream_ptr())
    return _deferred(None, workspace, bsz, vsrc, rows, cin, cout, DW_BF16)


def spiral_conv_bwd_rowsub_pair_bf16(x, idx, dpre, flat, w, dx, elu_y=None, workspace=None):
    """The bf16 step's Enblock backward in ONE launch
    (``cfsd_spiral_conv_bwd_rowsub_pair_bf16``, ABI 4.11): the dx of
    :func:`spiral_conv_bwd_data_rowsub` (fp32 batch-major ``dpre`` at the kept
    rows, fp32 ``w``; bf16 vertex-major ``dx`` / ``elu_y``) and the deferred
    slabs of :func:`spiral_conv_bwd_weight_x` (bf16 vertex-major ``x``);
    returns the DeferredDw."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    _need_vm(x, (bsz, vsrc, cin), "x", torch.bfloat16)
    _need_vm(dx, (bsz, vsrc, cin), "dx", torch.bfloat16)
    _need_like(dx, "dx", (bsz, vsrc, cin), torch.bfloat16, elu_y=elu_y)
    _need(dpre, (bsz, rows, cout), torch.float32, "dpre")
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, seq * cin), torch.float32, "w")
    workspace, nbytes = _conv_ws(_need(workspace, None, name="workspace"), x.device,
                                 spiral_conv_bwd_weight_x_workspace(bsz, rows, seq, cin, cout))
    call("cfsd_spiral_conv_bwd_rowsub_pair_bf16", ptr(x), ptr(idx), ptr(dpre), ptr(table), width, ptr(w),
         ptr(elu_y), ptr(dx), ptr(workspace), ctypes.c_size_t(nbytes), bsz, vsrc, rows, seq, cin, cout,
         stream_ptr())
    return _deferred(None, workspace, bsz, vsrc, rows, cin, cout, DW_BF16)


def spiral_conv_bwd_x(x, idx, dpre, inv, w, dw, db, dx=None, elu_y=None, workspace=None):
    """Fused dx + dW of the xyz output conv with bf16 (or fp32) x / elu_y /
    dx in either layout."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    xdt = x.dtype
    if xdt not in (torch.float32, torch.bfloat16):
        raise ValueError(f"x must be fp32 or bf16, got {xdt}")
    _needl(x, None, "x", xdt)
    _needl(dpre, (bsz, rows, cout), "dpre", torch.float32)
    inv_ptr, inv_row, inv_head = _need_inv(inv, vsrc, rows, seq)
    _need(w, (cout, seq * cin), name="w")
    _need_like(x, "x", (bsz, vsrc, cin), xdt, dx=dx, elu_y=elu_y)
    _need_dw_db(dw, db, cout, seq * cin)
    ws, nb = _conv_ws(workspace, x.device, spiral_conv_bwd_workspace(bsz, vsrc, rows, seq, cin, cout))
    call("cfsd_spiral_conv_bwd_x", ptr(x), _st(x), ptr(idx), ptr(dpre), _st(dpre), ptr(inv_ptr), ptr(inv_row),
         ptr(inv_head), ptr(w), ptr(elu_y), ptr(dx), ptr(dw), ptr(db), ptr(ws), ctypes.c_size_t(nb),
         bsz, vsrc, rows, seq, cin, cout, stream_ptr())
    return _with_dx(dx, _deferred(dw, ws, bsz, vsrc, rows, cin, cout, DW_FUSED))


def spiral_conv_bwd_out_flat(x, idx, dpre, flat, w, dw, db, dx=None, elu_y=None, workspace=None):
    """Fused dx + dW of the xyz output conv (32 -> 3) with vertex-major x /
    elu_y / dx (fp32 or bf16) and dpre, through the flat inverse list
    (``topology.spiral_flat``); batch a multiple of 16."""
    (bsz, vsrc, rows, seq, cin), cout = _conv_dims(x, idx), dpre.shape[2]
    xdt = x.dtype
    _need_vm(x, None, "x", xdt)
    _need_vm(dpre, (bsz, rows, cout), "dpre", torch.float32)
    table, width = _need_flat(flat, vsrc)
    _need(w, (cout, seq * cin), name="w")
    _need_like(x, "x", (bsz, vsrc, cin), xdt, dx=dx, elu_y=elu_y)
    _need_dw_db(dw, db, cout, seq * cin)
    ws, nb = _conv_ws(workspace, x.device, spiral_conv_bwd_workspace(bsz, vsrc, rows, seq, cin, cout))
    call("cfsd_spiral_conv_bwd_out_flat", ptr(x), _st(x), ptr(idx), ptr(dpre), _st(dpre), ptr(table), width,
         ptr(w), ptr(elu_y), ptr(dx), ptr(dw), ptr(db), ptr(ws), ctypes.c_size_t(nb), bsz, vsrc, rows, seq, cin,
         cout, stream_ptr())
    return _with_dx(dx, _deferred(dw, ws, bsz, vsrc, rows, cin, cout, DW_FUSED))


def spmm_x(csr, x, m, elu_y=None, out=None, order=None, uniform=0, sched=None):
    """Pool SpMM with fp32 or bf16 operands (fp32 sums, file order)."""
    row_ptr, col, val = csr
    bsz, n, c = x.shape
    _needl(x, None, "x")
    _need(row_ptr, (m + 1,), torch.int32, "row_ptr")
    _need(col, None, torch.int32, "col")
    _need(val, (col.numel(),), name="val")
    _needl(out, (bsz, m, c), "out")
    if elu_y is not None:
        _needl(elu_y, (bsz, m, c), "elu_y", out.dtype)
        _same_layout(out, elu_y, "out and elu_y")
    if sched is not None:
        _spmm_sched_csr(sched, x, elu_y, out, bsz, m, n, c)
        return out
    if order is not None:
        _spmm_sched(row_ptr, col, val, order, x, elu_y, out, bsz, m, n, c)
        return out
    if uniform:
        _spmm_uniform(uniform, col, val, x, elu_y, out, bsz, m, n, c)
        return out
    call("cfsd_spmm_csr_x", ptr(row_ptr), ptr(col), ptr(val), ptr(x), _st(x), ptr(elu_y), ptr(out),
         _st(out), bsz, m, n, c, stream_ptr())
    return out


# ------------------------------------------------------------------ t-SNE
TSNE_MAX_K, TSNE_MAX_D = _H["CFSD_TSNE_MAX_K"], _H["CFSD_TSNE_MAX_D"]
TSNE_KNN_ROWS, TSNE_KNN_COLS, TSNE_KNN_DIMS = (_H["CFSD_TSNE_KNN_ROWS"], _H["CFSD_TSNE_KNN_COLS"],
                                               _H["CFSD_TSNE_KNN_DIMS"])  # cfsd_knn_rows' tiling
TSNE_ROWS, TSNE_TILE = _H["CFSD_TSNE_ROWS"], _H["CFSD_TSNE_TILE"]  # the repulsive kernel's rows / staged columns
TSNE_MAX_SPLITS, TSNE_MAX_N = _H["CFSD_TSNE_MAX_SPLITS"], _H["CFSD_TSNE_MAX_N"]
TSNE_LONG_ROW, TSNE_ATT_ROWS = _H["CFSD_TSNE_LONG_ROW"], _H["CFSD_TSNE_ATT_ROWS"]  # the attractive kernel's


def _knn_limits(n, k, what):
    if n < 2:
        raise ValueError(f"{what}: {n} rows, at least 2")
    if not 1 <= k <= min(n - 1, TSNE_MAX_K):
        raise ValueError(f"{what}: k={k} outside 1..min(n - 1 = {n - 1}, {TSNE_MAX_K})")
    if n * k >= 2 ** 31:
        raise ValueError(f"{what}: n x k = {n * k} >= 2^31")


def knn_rows(z, k):
    """The ``k`` nearest other rows of every row of ``z`` ``[n, d]``
    (``cfsd_knn_rows``): ``(idx [n, k] int32, d2 [n, k] float32)``, squared
    Euclidean distances in difference form, each row sorted ascending by
    ``(d2, index)``; the row itself is excluded."""
    _need(z, None, name="z")
    if z.dim() != 2:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [n, d]")
    n, d, k = int(z.shape[0]), int(z.shape[1]), int(k)
    _knn_limits(n, k, "knn_rows")
    if not 1 <= d <= TSNE_MAX_D:
        raise ValueError(f"knn_rows: d={d} outside 1..{TSNE_MAX_D}")
    idx = torch.empty((n, k), dtype=torch.int32, device=z.device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=z.device)
    call("cfsd_knn_rows", ptr(z), ptr(idx), ptr(d2), None, ctypes.c_size_t(0), n, d, k, stream_ptr())
    return idx, d2


def tsne_affinities(d2, perplexity):
    """``_binary_search_perplexity`` (``sklearn/manifold/_utils.pyx``) on the
    device, in float64 (``cfsd_tsne_affinities``): ``d2`` ``[n, k]`` squared
    neighbour distances -> ``(p_cond [n, k], beta [n])`` float32, the
    conditional probabilities of the last precision the search evaluated and
    that precision."""
    _need(d2, None, name="d2")
    if d2.dim() != 2:
        raise ValueError(f"d2: shape {tuple(d2.shape)}, expected [n, k]")
    n, k = int(d2.shape[0]), int(d2.shape[1])
    _knn_limits(n, k, "tsne_affinities")
    perplexity = float(perplexity)
    if not 0.0 < perplexity < float("inf"):
        raise ValueError(f"perplexity {perplexity} is not a positive number")
    p_cond = torch.empty((n, k), dtype=torch.float32, device=d2.device)
    beta = torch.empty((n,), dtype=torch.float32, device=d2.device)
    call("cfsd_tsne_affinities", ptr(d2), ptr(p_cond), ptr(beta), n, k, perplexity, stream_ptr())
    return p_cond, beta


def tsne_symmetrize(idx, p_cond):
    """The second half of ``_joint_probabilities_nn`` (``sklearn/manifold/_t_sne.py``):
    ``P = (P_cond + P_cond^T) / sum`` of the kNN-sparse conditional
    probabilities ``idx`` / ``p_cond`` ``[n, k]``, as a CSR ``(row_ptr [n + 1]
    int32, col [nnz] int32 ascending within a row, val [nnz] float32)``.
    Float64 on the tensors' own device (CPU tensors are fine: torch only, no
    kernel); an entry is the sum of at most two terms, so no order is left
    open.  Entries that are exactly 0 are dropped, as scipy's sparse addition
    drops them."""
    if idx.dim() != 2 or idx.shape != p_cond.shape or idx.device != p_cond.device:
        raise ValueError(f"idx {tuple(idx.shape)} and p_cond {tuple(p_cond.shape)}: expected two [n, k] on one device")
    n, k = int(idx.shape[0]), int(idx.shape[1])
    rows = torch.arange(n, device=idx.device, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    if n < 2 or k < 1 or int(cols.min()) < 0 or int(cols.max()) >= n:
        raise ValueError("tsne_symmetrize: neighbour indices outside [0, n)")
    vals = p_cond.reshape(-1).to(torch.float64)
    keys, order = torch.sort(torch.cat([rows * n + cols, cols * n + rows]), stable=True)
    vals = torch.cat([vals, vals])[order]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = keys[1:] != keys[:-1]
    if int((~first[1:] & ~first[:-1]).sum()) != 0:
        raise ValueError("tsne_symmetrize: a row names one neighbour twice")
    twin = torch.zeros_like(vals)  # the transposed entry, where there is one, follows its key directly
    twin[:-1] = torch.where(first[1:], twin[:-1], vals[1:])
    keep = first & ((vals + twin) != 0)
    keys, val = keys[keep], (vals + twin)[keep]
    if keys.numel() >= 2 ** 31:
        raise ValueError(f"tsne_symmetrize: nnz = {keys.numel()} >= 2^31")
    total = torch.clamp(val.sum(), min=torch.finfo(torch.float64).eps)
    row_ptr = torch.searchsorted(keys, torch.arange(n + 1, device=keys.device, dtype=torch.int64) * n)
    return row_ptr.to(torch.int32), (keys % n).to(torch.int32), (val / total).to(torch.float32)


def tsne_joint_probabilities(z, perplexity=30.0):
    """``_joint_probabilities_nn`` of ``TSNE(method='barnes_hut')``: the
    ``k = min(n - 1, int(3 * perplexity + 1))`` nearest neighbours of every
    row of ``z`` ``[n, d]`` (:func:`knn_rows`), the perplexity search
    (:func:`tsne_affinities`) and the symmetrisation (:func:`tsne_symmetrize`)
    -> the CSR ``(row_ptr, col, val)`` of ``P``.  ``perplexity >= n`` is a
    ``ValueError``, as in scikit-learn."""
    if z is None or z.dim() != 2:
        raise ValueError("z: expected a tensor [n, d]")
    n, perplexity = int(z.shape[0]), float(perplexity)
    if not perplexity > 0.0:
        raise ValueError(f"perplexity {perplexity} is not a positive number")
    if perplexity >= n:
        raise ValueError("perplexity must be less than n_samples")
    _need(z, None, name="z")
    idx, d2 = knn_rows(z, min(n - 1, int(3.0 * perplexity + 1)))
    p_cond, _ = tsne_affinities(d2, perplexity)
    return tsne_symmetrize(idx, p_cond)


def tsne_splits(n):
    """``cfsd_tsne_splits``: the column splits per row block that ``splits=0``
    stands for; a function of ``n`` alone."""
    return int(_abi.lib().cfsd_tsne_splits(int(n)))


def tsne_workspace(n, splits=0, device="cuda"):
    """Scratch of one :func:`tsne_step` (``cfsd_tsne_step_workspace``)."""
    need = int(_abi.lib().cfsd_tsne_step_workspace(int(n), int(splits)))
    if need == 0:
        raise ValueError(f"tsne_workspace: n={n} or splits={splits} outside the supported range")
    return torch.empty(need // 4 + 1, dtype=torch.float32, device=device)


def tsne_step(y, update, gains, csr, momentum, learning_rate, exaggeration=1.0, splits=0, want_error=False,
              workspace=None, grad=None, result=None):
    """One iteration of ``_gradient_descent`` on ``_kl_divergence_bh(angle=0)``
    (``sklearn/manifold/_t_sne.py``), three launches and no synchronisation:
    the exact repulsive term, the attractive term over the CSR ``csr =
    (row_ptr, col, val)`` of ``P`` (times ``exaggeration``), ``grad = 4 (attr -
    rep / Z)`` and the gains / momentum rule, which updates ``y``, ``update``
    and ``gains`` ``[n, 2]`` IN PLACE.  ``splits``: column splits of the
    repulsive kernel (0 = :func:`tsne_splits`).  Returns ``grad`` ``[n, 2]``;
    with ``want_error`` ``(grad, result)``, ``result`` two device floats: the
    KL divergence and ``|gains * grad|`` as ``_gradient_descent`` checks them."""
    _need(y, None, name="y")
    if y.dim() != 2 or y.shape[1] != 2:
        raise ValueError(f"y: shape {tuple(y.shape)}, expected [n, 2]")
    n = int(y.shape[0])
    if not 2 <= n <= TSNE_MAX_N:
        raise ValueError(f"tsne_step: n={n} outside 2..{TSNE_MAX_N}")
    _need(update, (n, 2), name="update")
    _need(gains, (n, 2), name="gains")
    row_ptr, col, val = csr
    _need(row_ptr, (n + 1,), torch.int32, "row_ptr")
    _need(col, None, torch.int32, "col")
    nnz = int(col.numel())
    _need(col, (nnz,), torch.int32, "col")
    _need(val, (nnz,), name="val")
    splits = int(splits)
    if not 0 <= splits <= TSNE_MAX_SPLITS:
        raise ValueError(f"tsne_step: splits={splits} outside 0..{TSNE_MAX_SPLITS}")
    if not float(exaggeration) > 0.0:
        raise ValueError(f"tsne_step: exaggeration {exaggeration} <= 0")
    if workspace is None:
        workspace = tsne_workspace(n, splits, y.device)
    _need(workspace, None, name="workspace")
    nbytes = ctypes.c_size_t(workspace.numel() * workspace.element_size())
    grad = _out(grad, (n, 2), y, "grad")
    want = 1 if want_error else 0
    if want_error:
        result = _out(result, (2,), y, "result")
    call("cfsd_tsne_forces", ptr(y), ptr(row_ptr), ptr(col), ptr(val), ptr(workspace), nbytes, n, nnz, splits,
         float(exaggeration), want, stream_ptr())
    call("cfsd_tsne_update", ptr(y), ptr(update), ptr(gains), ptr(grad), ptr(result) if want_error else None,
         ptr(workspace), nbytes, n, splits, float(exaggeration), float(momentum), float(learning_rate), want,
         stream_ptr())
    return (grad, result) if want_error else grad


# ------------------------------------------------------------------ surgical planning
PLAN_MAX_LEVELS, PLAN_MAX_STEPS = _H["CFSD_PLAN_MAX_LEVELS"], _H["CFSD_PLAN_MAX_STEPS"]
PLAN_MAX_FIRST, PLAN_MAX_WINDOWS = _H["CFSD_PLAN_MAX_FIRST"], _H["CFSD_PLAN_MAX_WINDOWS"]


def _host_array(ctype, values):
    """A HOST argument of an entry point: a ctypes array and its address."""
    arr = (ctype * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _plan_levels(levels):
    levels = [float(v) for v in levels]
    if not 1 <= len(levels) <= PLAN_MAX_LEVELS:
        raise ValueError(f"{len(levels)} levels: 1..{PLAN_MAX_LEVELS} are supported")
    if any(not 0.0 < v < float("inf") for v in levels) or any(b >= a for a, b in zip(levels, levels[1:])):
        raise ValueError(f"levels {levels}: expected positive, finite, strictly descending numbers")
    return levels


def plan_targets(z, mean, whiten, levels=(3.0, 2.0, 1.0), steps=5000, cols=None):
    """The crossings of ``Tester.interpolate_syndrome_to_normal``
    (``test.py:663-704``) for every row of ``z`` ``[n, ld]`` at once
    (``cfsd_plan_targets``): ``mean`` ``[d]`` and ``whiten`` ``[d, d]`` are the
    healthy class of a QDA over the column window ``cols = (col0, d)``
    (default: every column), ``levels`` descending Mahalanobis radii, ``steps``
    the points of the ``torch.linspace`` from the row to ``mean``.  Returns
    ``(maha [n], index [n, S] int32, targets [n, S + 1, d])``: the row's
    distance, per level the first grid point within it (0 for a row already
    inside) and that point; ``targets[:, S]`` is ``mean``."""
    n, ld, col0, d = _window(z, cols)
    _need(mean, (d,), name="mean")
    _need(whiten, (d, d), name="whiten")
    if mean.device != z.device or whiten.device != z.device:
        raise ValueError(f"mean / whiten are on {mean.device} / {whiten.device}, z on {z.device}")
    levels, steps = _plan_levels(levels), int(steps)
    if not 2 <= steps <= PLAN_MAX_STEPS:
        raise ValueError(f"steps={steps} outside 2..{PLAN_MAX_STEPS}")
    s = len(levels)
    if n * ld >= 2 ** 31 or n * (s + 1) * d >= 2 ** 31:
        raise ValueError("plan_targets: n x ld or n x (levels + 1) x d >= 2^31")
    maha = torch.empty((n,), dtype=torch.float32, device=z.device)
    index = torch.empty((n, s), dtype=torch.int32, device=z.device)
    targets = torch.empty((n, s + 1, d), dtype=torch.float32, device=z.device)
    keep, lv = _host_array(ctypes.c_float, levels)
    call("cfsd_plan_targets", ptr(z), ptr(mean), ptr(whiten), lv, ptr(maha), ptr(index), ptr(targets), n, ld, col0, d,
         s, steps, stream_ptr())
    return maha, index, targets


def plan_tables(z, targets, mask=None, n_first=8):
    """The latent tables of ``test.py:706-740`` (``cfsd_plan_tables``): ``z``
    ``[n, L]``, ``targets`` ``[n, S + 1, L]`` of a full-width
    :func:`plan_targets`, ``mask`` ``[P, L]`` uint8 the columns each procedure
    moves (``None``: no procedure).  Returns ``(tables [n, 1 + P, n_first + S,
    L], dist [n, 1 + P, S + 1])``: group 0 moves every column (``n_first``
    rows from ``z`` to the first target, then the other targets), group ``1 +
    p`` only procedure ``p``'s columns; ``dist`` the mean squared distance of
    the last ``S + 1`` rows to ``targets[:, S]`` (``d3, d2, d1, dm``)."""
    _need(z, None, name="z")
    if z.dim() != 2 or z.shape[0] < 1 or not 1 <= z.shape[1] <= CLS_MAX_D:
        raise ValueError(f"z: shape {tuple(z.shape)}, expected [n >= 1, 1..{CLS_MAX_D}]")
    n, lat = int(z.shape[0]), int(z.shape[1])
    _need(targets, None, name="targets")
    if targets.dim() != 3 or targets.shape[0] != n or targets.shape[2] != lat or \
            not 2 <= targets.shape[1] <= PLAN_MAX_LEVELS + 1:
        raise ValueError(f"targets: shape {tuple(targets.shape)}, expected [{n}, 2..{PLAN_MAX_LEVELS + 1}, {lat}]")
    s = int(targets.shape[1]) - 1
    p = 0
    if mask is not None:
        _need(mask, None, torch.uint8, "mask")
        if mask.dim() != 2 or mask.shape[1] != lat:
            raise ValueError(f"mask: shape {tuple(mask.shape)}, expected [P, {lat}]")
        p = int(mask.shape[0])
    for name, t in (("targets", targets), ("mask", mask)):
        if t is not None and t.device != z.device:
            raise ValueError(f"{name} is on {t.device}, z on {z.device}")
    n_first = int(n_first)
    if not 1 <= n_first <= PLAN_MAX_FIRST:
        raise ValueError(f"n_first={n_first} outside 1..{PLAN_MAX_FIRST}")
    f = n_first + s
    if n * (1 + p) * f * lat >= 2 ** 31:
        raise ValueError("plan_tables: n x (1 + P) x frames x latent >= 2^31")
    tables = torch.empty((n, 1 + p, f, lat), dtype=torch.float32, device=z.device)
    dist = torch.empty((n, 1 + p, s + 1), dtype=torch.float32, device=z.device)
    call("cfsd_plan_tables", ptr(z), ptr(targets), ptr(mask) if p else None, ptr(tables), ptr(dist), n, lat, s, p,
         n_first, stream_ptr())
    return tables, dist


PAIR_RAW = ("maha_pre", "maha_post", "l2_pre", "l2_post", "cosine", "maha_displacement")  # raw[..., q]


def pair_metrics(z_pre, z_post, windows, mean, whiten):
    """The raw quantities of ``Tester.evaluate_pre_post_pair``
    (``test.py:992-1081``) for ``N`` pairs and ``W`` column windows in one
    launch (``cfsd_pair_metrics``): ``z_pre`` / ``z_post`` ``[N, L]``;
    ``windows`` a host sequence of ``(col0, d, mean offset, whiten offset)``
    into the packed device arrays ``mean`` / ``whiten`` (flat: per window the
    healthy mean ``[d]`` and whitening matrix ``[d, d]``).  Returns ``raw``
    ``[N, W, 6]`` in the order of ``PAIR_RAW``; the cosine of a zero
    displacement is NaN."""
    _need(z_pre, None, name="z_pre")
    if z_pre.dim() != 2 or z_pre.shape[0] < 1 or z_pre.shape[1] < 1:
        raise ValueError(f"z_pre: shape {tuple(z_pre.shape)}, expected [N >= 1, L >= 1]")
    n, lat = int(z_pre.shape[0]), int(z_pre.shape[1])
    _need(z_post, (n, lat), name="z_post")
    _need(mean, None, name="mean")
    _need(whiten, None, name="whiten")
    if mean.dim() != 1 or whiten.dim() != 1 or not mean.numel() or not whiten.numel():
        raise ValueError(f"mean {tuple(mean.shape)} / whiten {tuple(whiten.shape)}: expected two flat packed arrays")
    for name, t in (("z_post", z_post), ("mean", mean), ("whiten", whiten)):
        if t.device != z_pre.device:
            raise ValueError(f"{name} is on {t.device}, z_pre on {z_pre.device}")
    rows = [tuple(int(v) for v in w) for w in windows]
    if not 1 <= len(rows) <= PLAN_MAX_WINDOWS or any(len(w) != 4 for w in rows):
        raise ValueError(f"{len(rows)} windows: 1..{PLAN_MAX_WINDOWS} rows of (col0, d, mean offset, whiten offset)")
    for i, (col0, d, mo, wo) in enumerate(rows):
        if col0 < 0 or d < 1 or col0 + d > lat or d > CLS_MAX_D:
            raise ValueError(f"window {i}: columns [{col0}, {col0 + d}) outside [0, {lat}) or wider than {CLS_MAX_D}")
        if mo < 0 or mo + d > mean.numel() or wo < 0 or wo + d * d > whiten.numel():
            raise ValueError(f"window {i}: offsets {mo} / {wo} past the packed mean ({mean.numel()}) or whiten "
                             f"({whiten.numel()})")
    if n * lat >= 2 ** 31 or n * len(rows) * 6 >= 2 ** 31 or max(mean.numel(), whiten.numel()) >= 2 ** 31:
        raise ValueError("pair_metrics: n x L, n x W x 6 or a packed array >= 2^31")
    raw = torch.empty((n, len(rows), 6), dtype=torch.float32, device=z_pre.device)
    keep, win = _host_array(ctypes.c_int32, [v for w in rows for v in w])
    call("cfsd_pair_metrics", ptr(z_pre), ptr(z_post), win, ptr(mean), ptr(whiten), ptr(raw), n, lat, len(rows),
         int(mean.numel()), int(whiten.numel()), stream_ptr())
    return raw


# ------------------------------------------------------------------ embedding figures
KDE_CHUNK, KDE_MAX_G = _H["CFSD_KDE_CHUNK"], _H["CFSD_KDE_MAX_G"]  # points per LDS chunk of cfsd_kde2d; largest grid side
PRIM_ROUND, PRIM_FLOATS, PRIM_MAX = _H["CFSD_PRIM_ROUND"], _H["CFSD_PRIM_FLOATS"], _H["CFSD_PRIM_MAX"]
PRIM_DISC, PRIM_SEGMENT, PRIM_TRIANGLE = _H["CFSD_PRIM_DISC"], _H["CFSD_PRIM_SEGMENT"], _H["CFSD_PRIM_TRIANGLE"]
FIG_MAX_SIZE = _H["CFSD_FIG_MAX_SIZE"]
SHADE_MAX_PANELS, SHADE_MAX_LAYERS = _H["CFSD_SHADE_MAX_PANELS"], _H["CFSD_SHADE_MAX_LAYERS"]
SHADE_MAX_LEVELS = _H["CFSD_SHADE_MAX_LEVELS"]
SHADE_PANEL_DOUBLES, SHADE_LAYER_DOUBLES = _H["CFSD_SHADE_PANEL_DOUBLES"], _H["CFSD_SHADE_LAYER_DOUBLES"]


def _host_table(values, dtype, cols, name):
    """A HOST table of an entry point: a C-contiguous NumPy array ``[rows,
    cols]`` (``cols`` None: flat) and its address; keep the array alive over
    the call."""
    import numpy as np
    arr = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    if (cols is None and arr.ndim != 1) or (cols is not None and (arr.ndim != 2 or arr.shape[1] != cols)):
        raise ValueError(f"{name}: shape {arr.shape}, expected " + ("[n]" if cols is None else f"[n, {cols}]"))
    return arr, ctypes.c_void_p(arr.ctypes.data)


def kde2d(points, set_ptr, params, grid_size):
    """``S`` Gaussian kernel density estimates on ``grid_size`` x ``grid_size``
    grids in one call (``cfsd_kde2d``), float64 throughout: ``points`` ``[N,
    2]`` float64 (device) grouped by set through the host sequence ``set_ptr``
    ``[S + 1]``; ``params`` a host table ``[S, 8]`` per set of ``L00, L10, L11``
    (the lower-triangular factor of the inverse kernel covariance), ``scale``,
    ``lo0, step0, lo1, step1``.  Returns ``density`` ``[S, G, G]``:
    ``density[s, i, j] = scale * sum_k exp(-|L^T (g_ij - x_k)|^2 / 2)``, the sum
    in point order; zeros for an empty set."""
    import numpy as np
    _need(points, None, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 2:
        raise ValueError(f"points: shape {tuple(points.shape)}, expected [N, 2]")
    n, g = int(points.shape[0]), int(grid_size)
    sp, sp_p = _host_table(set_ptr, np.int32, None, "set_ptr")
    if sp.size < 2:
        raise ValueError("set_ptr: at least one set is required")
    s = sp.size - 1
    if sp[0] < 0 or sp[-1] > n or np.any(np.diff(sp) < 0):
        raise ValueError(f"set_ptr must ascend within [0, {n}]")
    par, par_p = _host_table(params, np.float64, 8, "params")
    if par.shape[0] != s:
        raise ValueError(f"params: {par.shape[0]} rows for {s} sets")
    if not np.all(np.isfinite(par)) or np.any(par[:, 5] <= 0) or np.any(par[:, 7] <= 0):
        raise ValueError("params must be finite, with positive grid steps")
    if not 2 <= g <= KDE_MAX_G:
        raise ValueError(f"grid_size={g} outside 2..{KDE_MAX_G}")
    if n >= 2 ** 30 or s * g * g >= 2 ** 31:
        raise ValueError("kde2d: N >= 2^30 or S x G x G >= 2^31")
    density = torch.empty((s, g, g), dtype=torch.float64, device=points.device)
    call("cfsd_kde2d", ptr(points) if n else None, sp_p, par_p, ptr(density), n, s, g, stream_ptr())
    return density


def density_shade(image, grids, panels, layers):
    """Shade density layers into ``image`` ``[3, H, W]`` fp32 in place
    (``cfsd_density_shade``): ``grids`` a flat float64 device tensor holding the
    density grids; ``panels`` a host table ``[P, 8]`` of ``px0, py0, pw, ph,
    xlo, xhi, ylo, yhi``; ``layers`` a host table ``[n, 24]`` of ``panel, grid
    offset, G0, G1, lo0, step0, lo1, step1, K, 8 levels, r, g, b, a, fill, line,
    0`` (``include/cfsd.h`` states the arithmetic).  Layers apply in order;
    pixels outside every panel are not written.  Returns ``image``."""
    import numpy as np
    _need(image, None, name="image")
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image: shape {tuple(image.shape)}, expected [3, H, W]")
    h, w = int(image.shape[1]), int(image.shape[2])
    if not (1 <= h <= FIG_MAX_SIZE and 1 <= w <= FIG_MAX_SIZE):
        raise ValueError(f"image {h} x {w}: sides of 1..{FIG_MAX_SIZE} are supported")
    _need(grids, None, torch.float64, "grids")
    if grids.dim() != 1 or grids.numel() < 4 or grids.numel() >= 2 ** 31 or grids.device != image.device:
        raise ValueError(f"grids: expected a flat float64 tensor of 4..2^31 values on {image.device}")
    pan, pan_p = _host_table(panels, np.float64, SHADE_PANEL_DOUBLES, "panels")
    lay, lay_p = _host_table(layers, np.float64, SHADE_LAYER_DOUBLES, "layers")
    if not 1 <= pan.shape[0] <= SHADE_MAX_PANELS:
        raise ValueError(f"{pan.shape[0]} panels: 1..{SHADE_MAX_PANELS} are supported")
    if not 1 <= lay.shape[0] <= SHADE_MAX_LAYERS:
        raise ValueError(f"{lay.shape[0]} layers: 1..{SHADE_MAX_LAYERS} are supported")
    k = lay[:, 8]
    if np.any(k != np.floor(k)) or np.any(k < 1) or np.any(k > SHADE_MAX_LEVELS):
        raise ValueError(f"layers: K outside 1..{SHADE_MAX_LEVELS}")
    call("cfsd_density_shade", ptr(image), ptr(grids), pan_p, lay_p, h, w, pan.shape[0], lay.shape[0],
         int(grids.numel()), stream_ptr())
    return image


def draw_primitives(images, prims, prim_ptr):
    """Composite discs, segments and triangles into ``images`` ``[B, 3, H, W]``
    fp32 in place (``cfsd_draw_primitives``): ``prims`` a host table ``[n, 16]``
    of ``kind, x0, y0, x1, y1, x2, y2, r, red, green, blue, alpha, clip x0, y0,
    x1, y1`` (``PRIM_DISC`` / ``PRIM_SEGMENT`` / ``PRIM_TRIANGLE``, pixels),
    ``prim_ptr`` the host sequence ``[B + 1]``: image ``b`` takes the rows
    ``prim_ptr[b] .. prim_ptr[b + 1]`` in order.  The tables are copied to the
    device here.  Returns ``images``."""
    import numpy as np
    _need(images, None, name="images")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images: shape {tuple(images.shape)}, expected [B, 3, H, W]")
    b, _, h, w = (int(v) for v in images.shape)
    if not (1 <= h <= FIG_MAX_SIZE and 1 <= w <= FIG_MAX_SIZE):
        raise ValueError(f"images {h} x {w}: sides of 1..{FIG_MAX_SIZE} are supported")
    if not 1 <= b <= 65535 or images.numel() >= 2 ** 31:
        raise ValueError(f"images: B={b} outside 1..65535, or B x 3 x H x W >= 2^31")
    pp, pp_p = _host_table(prim_ptr, np.int32, None, "prim_ptr")
    pr, pr_p = _host_table(np.asarray(prims, dtype=np.float32).reshape(-1, PRIM_FLOATS), np.float32, PRIM_FLOATS,
                           "prims")
    n = pr.shape[0]
    if pp.size != b + 1 or pp[0] < 0 or pp[-1] > n or np.any(np.diff(pp) < 0):
        raise ValueError(f"prim_ptr: expected {b + 1} ascending entries within [0, {n}]")
    if n > PRIM_MAX:
        raise ValueError(f"{n} primitives: at most {PRIM_MAX} are supported")
    if n:
        clip = pr[:, 12:16]
        if np.any(clip != np.floor(clip)) or np.any(clip[:, :2] < 0) or np.any(clip[:, 2] > w) or \
                np.any(clip[:, 3] > h) or np.any(clip[:, 2] < clip[:, 0]) or np.any(clip[:, 3] < clip[:, 1]):
            raise ValueError(f"prims: a clip rectangle lies outside the {h} x {w} image")
    d_pp = torch.from_numpy(pp).to(images.device)
    d_pr = torch.from_numpy(pr).to(images.device) if n else None
    call("cfsd_draw_primitives", ptr(images), ptr(d_pr), ptr(d_pp), pr_p if n else None, pp_p, b, h, w, n,
         stream_ptr())
    return images
