"""The fp32 vertex-major SpiralConv entry points (``cfsd_spiral_conv_fwd_x`` / ``_bwd_weight_x`` /
``_bwd_data_flat`` / ``_bwd_flat_pair`` / ``_bwd_out_flat`` / ``_bwd_x`` with fp32 or mixed operands;
``spiral_conv_vm32.hip``, ``dx_flat_vm32.h`` and the ``_x`` / ``_flat`` / ``_pair`` dispatch of
``spiral_conv.hip``) on the synthetic spiral tables of ``tests/golden/spiral_tables.py`` against the fp64
restatement of ``conv_cases.Case``, at the sizes where the dispatch changes kernel.  The bf16 MFMA kernels
are in ``test_gpu_bf16_conv.py``; the step-level and layout-agreement tests stay in ``test_gpu_vm32.py``.

Every case runs in TWO input modes:

  exact   every operand from a small dyadic set (``tests/golden/exact_values.py``): every product is a
          multiple of 1/4 and every partial sum stays below 2^22, so the result is the same in every
          summation order and in every MFMA-internal order.  fp32 results must EQUAL the restatement
          (``torch.equal``), bf16 results the restatement rounded to nearest even; the ELU branch of a
          forward is within one unit in the last place (``conv_cases.compare_elu_fwd``).  A lost list entry,
          an unwritten row, a swapped slot cannot hide under a rounding bound here.
  randn   ``randn`` operands against per-element bounds: a kernel that rounds where it should not, or that
          swaps two rows which coincide among the few exact values, shows here.

Bounds of the randn mode (per element; gamma_n = n u / (1 - n u), u = 2^-24, as derived in
``test_gpu_general_conv`` / ``test_gpu_specialised_conv``; re-derived per kernel from its code):

    forward   n = 9 cin + 1.  conv_fwd_vm32 and conv_fwd_lat: one fp32 MFMA chain over the 9 cin products, then
              the bias; the coarse conv_fwd_ks / conv_fwd_pt with a vertex-major x: per-slot-group chains and
              the LDS sum, at most cin + 9 roundings per term (test_gpu_specialised_conv).  conv_fwd_out_vm:
              36 fmafs per lane, the xor tree over 8 lanes (3 adds), the bias: 40 <= 9 * 32 + 1.  The xyz
              input conv (conv_fwd_in_mfma, K = 27 padded): 27 + 1.
    flat dx   n(u) = E(u) cout: conv_dx_flat_vm32 chains cout MFMA steps per list entry into ONE accumulator
              over the E(u) entries of the flat list, in list order (dx_flat_vm32.h); a padding entry adds
              nothing.  The same body is the dx half of conv_bwd_vm_pair.  With a bf16 dx (the bf16 step's
              Enblock, test_gpu_bf16_conv) the fp32 sum is rounded once on store.
    dW / db   n = batch * rows: conv_dw_lat / conv_dw_mfma with layout flags and conv_dw_vm32 sum one product
              per (mesh, row); units, ranges, slabs and the slab reduce are one summation tree over them.
    fused out conv_bwd_out_vm (32 -> 3, flat list): T_s[u, o] adds the list's rows of slot s (E_s - 1 adds),
              then a chain of 27 products: at most E(u) cout roundings, the flat-list count.  dW sums
              T_s[u, o] x[u, c] over (vertex, mesh): no more operations with a non-zero operand than
              batch * rows (test_gpu_specialised_conv's argument for the batch-major kernel); db sums the
              slot-0 list sums: every row is on exactly one slot-0 list.  bwd_fused_small with bf16
              operands (cfsd_spiral_conv_bwd_x): the inverse-table count max_s E_s - 1 + cout S.
    ELU/ELU'  one more u; a bf16 result one more 2^-8 (|ref| + tol).

Every output and workspace is pre-filled with NaN and a non-finite result refused; a second call is asserted
bit-identical; the deferred weight gradient (``dw is db is None``, then ``ops.dw_reduce_batch``) is asserted
bit-identical to the immediate one; ``elu_edges`` puts ELU' = 0 entries into every case, and the ``head_edge``
and ``fan`` tables absent vertices: both must give exactly 0.

Which branch a case takes, from the launchers' constants (M = batch * rows):

    case (batch x vsrc, rows = vsrc unless given)   constant it sits next to          forward (32 -> 32 / 32 -> 64)
    ---------------------------------------------   -------------------------------   -------------------------------
    16 x 37                                         --                                conv_fwd_ks with xvm
    16 x 511 / 513      M = 8176 / 8208             coarse::kMaxTilesFew * 16 = 8192  conv_fwd_ks / conv_fwd_pt, xvm
    16 x 1535 / 1537    M = 24560 / 24592           coarse::kMaxRows = 24576          conv_fwd_pt / launch_fwd_lat_x
                                                                                      (32 -> 32), conv_fwd_vm32<1,2>
                                                                                      (32 -> 64)
    16 x 4095 / 4097    M = 65520 / 65552           kLatFwdMax = kLatDwMax = 65536    32 -> 32: launch_fwd_lat_x /
                                                                                      conv_fwd_vm32<.,.,.,1,2>; dW
                                                                                      conv_dw_lat / conv_dw_vm32
                                                                                      (vm, vm, 32 -> 32) or
                                                                                      conv_dw_mfma with flags
    16 x 8191 / 8193    units = 8191 / 8193         kVm32Upt1Units = 8192             conv_fwd_vm32<.,.,.,1,2> /
                                                                                      <.,.,.,2,1>
    32 x 149, 48 x 149                              batch / 16 = 2, 3                 conv_fwd_ks with two and three
                                                                                      mesh groups per vertex
    48 x 1367           M = 65616                   kLatDwMax                         conv_fwd_vm32; dW as 16 x 4097
    16 x 2731 rows 683, 16 x 911 rows 2733          --                                conv_fwd_pt (M = 10928),
                                                                                      launch_fwd_lat_x / vm32 (43728)

``fwd_branch`` / ``dw_branch`` restate those conditions and every case asserts the branch it was written for;
the slab code of a weight gradient is the library's own (``cfsd_spiral_conv_bwd_weight_x_slabs``), the pair's
availability its workspace query.

Tables: the inverse-list-free kernels here read the forward table only, so ``hubs`` and ``head_edge`` differ in
fan-in and absent vertices; the rows != vsrc lines also run ``random`` and ``one_vertex_rows``.  The flat-list
kernels run ``fan_table(rows, vsrc, fan)`` with fan = the width (every padding of the last int4 group: fan,
fan - 1, fan - 2, fan - 3 entries on four neighbouring vertices); width 8 needs rows < vsrc (the mean fan-in of
a full table is 9).

Measured on an MI355X (largest err / bound of the randn mode; DESIGN.md section 15 has the full table):
forward ks 0.005, pt 0.006, lat 0.014, conv_fwd_vm32<1,2> 0.025, <2,1> 0.024, conv_fwd_out_vm 0.005; flat dx and the
pair's dx 0.135; dW lat 0.001, mfma / vm32 / pair below 0.001; conv_bwd_out_vm dx 0.673 with fp32 x (chains of three
terms per entry: few roundings, so the worst case is nearly met) and 0.996 with bf16 x (the store's own rounding
against 2^-8 |ref|); xyz input conv with a bf16 y 0.995 (the store), its dW 0.004; bwd_fused_small bf16 dx 0.996.
Exact mode: ELU branch at most 0.24 .. 0.49 of 2^-23.

Found by these tests and fixed: ``cfsd_spiral_conv_bwd_weight_x`` asked an fp32 x for the bf16 kernels' workspace
(larger than the fp32 slab set just below kLatDwMax rows), so the 16 x 4095 weight gradient with a workspace of
``ops.spiral_conv_bwd_weight_x_workspace(..., torch.float32)`` was refused; those cases are its regression test.

Not covered, with the reason:
  * conv_bwd_out_vm<., 8>: cfsd_spiral_conv_bwd_out_flat refuses vsrc != rows, and a table with rows == vsrc has
    mean fan-in 9, so its flat width is at least 12.
  * a 64-channel input in the fp32 vertex-major forward above coarse::kMaxRows: vm32::launch_fwd refuses it
    (asserted); below, conv_fwd_ks / conv_fwd_pt take it and are covered at 32 x 149 (64 -> 32, 64 -> 64).
  * conv_fwd_out_vm with U != 1 and the prefetch variants of conv_fwd_vm32 other than <1, 2> and <2, 1>:
    compile-time constants (kVmOutU, kVm32Pd2) pick one instance each.
  * vm32::conv_bwd_flat_pair / launch_dx_flat_b16 behind cfsd_spiral_conv_bwd_rowsub / _bwd_data_rowsub:
    covered by test_gpu_specialised_conv's row-subset tests (fp32) and test_gpu_bf16_conv (bf16 dx).
"""
import ctypes

import pytest
import torch

import spiral_tables as T
from conv_cases import (ACT_ELU, ACT_NONE, DEV, SEQ, assert_exact_zeros, compare, compare_elu_fwd, gamma,
                        make_conv_case, nan_out, nan_ws, same)
from craniofacialsd_vae_amd import _abi, ops, topology

pytestmark = pytest.mark.gpu

MODES = ("exact", "randn")
KS_MAX, PT_MAX, LAT_MAX, UPT1 = 512 * 16, 24576, 65536, 8192
BOTH = ("hubs", "head_edge")


def fwd_branch(batch, rows, cin, cout):
    """The kernel ``cfsd_spiral_conv_fwd_x`` runs for an fp32 vertex-major x (module docstring)."""
    m = batch * rows
    if m < PT_MAX:
        return "ks" if m < KS_MAX else "pt"
    if cin != 32:
        return "refused"
    if m < LAT_MAX and cout == 32:
        return "lat"
    return "vm32-1" if rows * (batch // 16) < UPT1 else "vm32-2"


def dw_branch(batch, rows, cin, cout, xvm, dpvm):
    if batch * rows < LAT_MAX:
        return "lat"
    return "vm32" if xvm and dpvm and cin == 32 and cout == 32 and batch % 16 == 0 else "mfma"


# ------------------------------------------------------------------ forward and weight gradient
def fwd_x(c, act, xvm, yvm, x_bf16=False, y_bf16=False):
    batch, vsrc, rows, seq, cin, cout = c.shape
    y = nan_out((batch, rows, cout), y_bf16, yvm)
    ops.spiral_conv_fwd_x(c.dev("x", x_bf16, xvm), c.d["idx"], c.d["w"], None, c.d["b"], act, y)
    assert ops.is_vm(y) == (yvm and batch > 1)
    return y


def check_fwd(c, cd, y, act, tag):
    if act == ACT_NONE:
        return compare(tag, y, cd.pre, cd.tol_fwd(), c.shape, c.exact)
    return compare_elu_fwd(tag + "+elu", y, cd.pre, cd.tol_fwd(), c.shape, c.exact)


def dw_x(c, xvm, dpvm, deferred, x_bf16=False, dp_bf16=False):
    batch, vsrc, rows, seq, cin, cout = c.shape
    x, dp = c.dev("x", x_bf16, xvm), c.dev("dpre", dp_bf16, dpvm)
    need = ops.spiral_conv_bwd_weight_x_workspace(batch, rows, seq, cin, cout, x.dtype)
    assert need > 0
    dw, db = nan_out((cout, seq * cin)), nan_out((cout,))
    if not deferred:
        assert ops.spiral_conv_bwd_weight_x(x, c.d["idx"], dp, dw, db, nan_ws(need)) is None
    else:
        item = ops.spiral_conv_bwd_weight_x(x, c.d["idx"], dp, None, None, nan_ws(need))
        assert isinstance(item, ops.DeferredDw)
        ops.dw_reduce_batch([(item, dw, db)])
    return dw, db


def dw_case(c, cd, xvm, dpvm, tag, **kw):
    """Immediate, deferred (bit-identical) and a second call (bit-identical) of one layout pair."""
    dw, db = dw_x(c, xvm, dpvm, False, **kw)
    compare(tag + " dw", dw, cd.dw, cd.tol_dw(), c.shape, c.exact)
    compare(tag + " db", db, cd.db, cd.tol_db(), c.shape, c.exact)
    for deferred in (True, False):
        dw2, db2 = dw_x(c, xvm, dpvm, deferred, **kw)
        assert torch.equal(dw2, dw) and torch.equal(db2, db), (tag, c.shape, deferred)


S3232, S3264, S6432, S6464 = (32, 32), (32, 64), (64, 32), (64, 64)
# (batch, vsrc, rows, tables, shapes)
FWD_DW_CASES = [
    (16, 37, 37, ("head_edge",), (S3232, S3264)),
    (16, 511, 511, BOTH, (S3232, S3264)),
    (16, 513, 513, BOTH, (S3232, S3264)),
    (16, 1535, 1535, BOTH, (S3232, S3264)),
    (16, 1537, 1537, BOTH, (S3232, S3264)),
    (16, 4095, 4095, BOTH, (S3232, S3264, S6432)),
    (16, 4097, 4097, BOTH, (S3232, S3264, S6432)),
    (16, 8191, 8191, BOTH, (S3232, S3264)),
    (16, 8193, 8193, BOTH, (S3232, S3264)),
    (32, 149, 149, ("head_edge",), (S3232, S3264, S6432, S6464)),
    (48, 149, 149, ("head_edge",), (S3232, S3264)),
    (48, 1367, 1367, BOTH, (S3232, S3264, S6432)),
    (16, 2731, 683, BOTH + ("random", "one_vertex_rows"), (S3232, S3264)),
    (16, 911, 2733, BOTH + ("random", "one_vertex_rows"), (S3232, S3264)),
]
FWD_DW_PARAMS = [pytest.param(b, v, r, t, ci, co, m, id=f"{b}x{v}-rows{r}-{ci}to{co}-{t}-{m}")
                 for b, v, r, tables, shapes in FWD_DW_CASES for t in tables for ci, co in shapes for m in MODES]
# the branch each size was chosen for (32 -> 32, 32 -> 64)
FWD_WANT = {(16, 37): ("ks", "ks"), (16, 511): ("ks", "ks"), (16, 513): ("pt", "pt"), (16, 1535): ("pt", "pt"),
            (16, 1537): ("lat", "vm32-1"), (16, 4095): ("lat", "vm32-1"), (16, 4097): ("vm32-1", "vm32-1"),
            (16, 8191): ("vm32-1", "vm32-1"), (16, 8193): ("vm32-2", "vm32-2"), (32, 149): ("ks", "ks"),
            (48, 149): ("ks", "ks"), (48, 1367): ("vm32-1", "vm32-1"), (16, 683): ("pt", "pt"),
            (16, 2733): ("lat", "vm32-1")}


@pytest.mark.parametrize("batch,vsrc,rows,table,cin,cout,mode", FWD_DW_PARAMS)
def test_forward_and_weight_gradient_fp32(batch, vsrc, rows, table, cin, cout, mode):
    """``ops.spiral_conv_fwd_x`` with a vertex-major fp32 x (y in both layouts, both activations) and
    ``ops.spiral_conv_bwd_weight_x`` with x / dpre vertex-major, mixed both ways."""
    c = make_conv_case(batch, vsrc, rows, cin, cout, table, mode, parts=("fwd", "dw"))
    cd = c.on_device()
    assert ops.spiral_conv_vm_has_shape(SEQ, cin, cout)
    branch = fwd_branch(batch, rows, cin, cout)
    if cin == 32:
        assert branch == FWD_WANT[(batch, rows)][cout == 64]
    if branch == "refused":   # a 64-channel input above the coarse kernels' range
        with pytest.raises(_abi.CfsdError):
            fwd_x(c, ACT_ELU, True, True)
    else:
        for yvm in (True, False):
            for act in (ACT_NONE, ACT_ELU):
                y = fwd_x(c, act, True, yvm)
                check_fwd(c, cd, y, act, f"fwd_x vm32 [{branch}]")
                assert same(fwd_x(c, act, True, yvm), y)
    lib = _abi.lib()
    for xvm, dpvm in ((True, True), (True, False), (False, True)):
        kind = dw_branch(batch, rows, cin, cout, xvm, dpvm)
        code = lib.cfsd_spiral_conv_bwd_weight_x_slabs(ops._st(c.dev("x", vm=xvm)), ops._st(c.dev("dpre", vm=dpvm)),
                                                       batch, cin, cout)
        assert code == (ops.DW_VM32 if xvm and dpvm and (cin, cout) == S3232 else ops.DW_PLAIN)
        dw_case(c, cd, xvm, dpvm, f"dw_x fp32 [{kind}]")


def test_forward_refuses_a_bf16_output_for_an_fp32_input():
    c = make_conv_case(16, 37, 37, 32, 32, "head_edge", "exact")
    with pytest.raises(_abi.CfsdError):
        fwd_x(c, ACT_NONE, True, True, y_bf16=True)


# ------------------------------------------------------------------ flat-list data gradient and the pair
def flat_dx(c, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ey = c.dev("elu_y", vm=True) if elu else None
    return ops.spiral_conv_bwd_data_flat(c.dev("dpre", vm=True), c.flat, c.d["w"], vsrc, elu_y=ey,
                                         out=nan_out((batch, vsrc, cin), vm=True))


def flat_pair(c, elu, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ws = nan_ws(ops.spiral_conv_bwd_flat_pair_workspace(batch, rows, seq, cin, cout))
    dx, dw, db = nan_out((batch, vsrc, cin), vm=True), nan_out((cout, seq * cin)), nan_out((cout,))
    ey = c.dev("elu_y", vm=True) if elu else None
    args = (c.dev("x", vm=True), c.d["idx"], c.dev("dpre", vm=True), c.flat, c.d["w"])
    if not deferred:
        assert ops.spiral_conv_bwd_flat_pair(*args, dw, db, dx, elu_y=ey, workspace=ws) is None
    else:
        item = ops.spiral_conv_bwd_flat_pair(*args, None, None, dx, elu_y=ey, workspace=ws)
        assert isinstance(item, ops.DeferredDw)
        ops.dw_reduce_batch([(item, dw, db)])
    return dx, dw, db


def dx_ref(cd, elu, tol):
    return cd.with_elu_grad(cd.dx, tol) if elu else (cd.dx, tol)


# (batch, vsrc, rows, fans): width 8 only where rows < vsrc
FLAT_CASES = [
    (16, 149, 149, (12, 16, 20)), (16, 149, 111, (8,)),
    (48, 149, 149, (12, 16, 20)), (48, 149, 111, (8,)),
    (16, 3644, 3644, (12, 16, 20)), (16, 3644, 2733, (8,)),
    (16, 4097, 4097, (12, 16, 20)), (16, 5500, 4100, (8,)),
    (48, 1367, 1367, (12, 16, 20)),
]
FLAT_PARAMS = [pytest.param(b, v, r, f, co, m, id=f"{b}x{v}-rows{r}-32to{co}-fan{f}-{m}")
               for b, v, r, fans in FLAT_CASES for f in fans for co in (32, 64) for m in MODES]


@pytest.mark.parametrize("batch,vsrc,rows,fan,cout,mode", FLAT_PARAMS)
def test_flat_list_data_gradient_and_pair_fp32(batch, vsrc, rows, fan, cout, mode):
    """``ops.spiral_conv_bwd_data_flat`` (conv_dx_flat_vm32<32, cout, width>) at every width, and for 32 -> 32
    ``ops.spiral_conv_bwd_flat_pair`` (conv_bwd_vm_pair<width>): from batch * rows = 65536 on it runs; below,
    its workspace query returns 0 and the call is refused."""
    paired = cout == 32 and batch * rows >= LAT_MAX
    c = make_conv_case(batch, vsrc, rows, 32, cout, "fan", mode, fan=fan, parts=("dx", "dw") if paired else ("dx",))
    cd = c.on_device()
    assert c.flat is not None and c.flat[1] == fan
    for elu in (False, True):
        ref, tol = dx_ref(cd, elu, cd.tol_dx())
        dx = flat_dx(c, elu)
        assert ops.is_vm(dx)
        compare("dx flat vm32" + ("*elu'" if elu else ""), dx, ref, tol, c.shape, c.exact)
        assert_exact_zeros(c, dx, elu)
        assert same(flat_dx(c, elu), dx)
    if cout != 32:
        assert ops.spiral_conv_bwd_flat_pair_workspace(batch, rows, SEQ, 32, cout) == 0
        return
    need = ops.spiral_conv_bwd_flat_pair_workspace(batch, rows, SEQ, 32, 32)
    if batch * rows < LAT_MAX:
        assert need == 0
        with pytest.raises(ValueError):
            flat_pair(c, False, False)
        ws, dxo = nan_ws(1 << 20), nan_out((batch, vsrc, 32), vm=True)
        with pytest.raises(_abi.CfsdError):   # the library itself refuses, before any launch
            ops.call("cfsd_spiral_conv_bwd_flat_pair", ops.ptr(c.dev("x", vm=True)), ops.ptr(c.d["idx"]),
                     ops.ptr(c.dev("dpre", vm=True)), ops.ptr(c.flat[0]), c.flat[1], ops.ptr(c.d["w"]), None,
                     ops.ptr(dxo), None, None, ops.ptr(ws), ctypes.c_size_t(ws.numel() * 4), batch, vsrc, rows, SEQ,
                     32, 32, ops.stream_ptr())
        assert bool(torch.isnan(dxo).all())
        return
    assert need > 0
    for elu in (False, True):
        ref, tol = dx_ref(cd, elu, cd.tol_dx())
        dx, dw, db = flat_pair(c, elu, False)
        compare("pair vm32 dx" + ("*elu'" if elu else ""), dx, ref, tol, c.shape, c.exact)
        compare("pair vm32 dw", dw, cd.dw, cd.tol_dw(), c.shape, c.exact)
        compare("pair vm32 db", db, cd.db, cd.tol_db(), c.shape, c.exact)
        assert_exact_zeros(c, dx, elu)
        for deferred in (True, False):
            dx2, dw2, db2 = flat_pair(c, elu, deferred)
            assert same(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize("width", [4, 24])
def test_flat_list_entry_points_refuse_other_widths(width):
    """Width 4 has no full-table instance and a fan-in of 21 no table at all (``inverse_flat`` gives none;
    a hand-made width-24 table is refused)."""
    c = make_conv_case(16, 149, 111, 32, 32, "fan", "exact", fan=8)
    table = torch.full((149, width), -1, dtype=torch.int32, device=DEV)
    table[:, :min(width, 8)] = c.flat[0][:, :min(width, 8)]
    c.flat = (table, width)
    with pytest.raises(_abi.CfsdError):
        flat_dx(c, False)
    big = make_conv_case(16, 5500, 4100, 32, 32, "fan", "exact", fan=8)
    assert ops.spiral_conv_bwd_flat_pair_workspace(16, 4100, SEQ, 32, 32) > 0
    t2 = torch.full((5500, width), -1, dtype=torch.int32, device=DEV)
    big.flat = (t2, width)
    with pytest.raises(_abi.CfsdError):
        flat_pair(big, False, False)
    assert topology.inverse_flat(T.fan_table(149, 149, 21, seed=21), 149, max_width=20) == (None, 0)


def test_flat_list_data_gradient_refuses_batch_24():
    c = make_conv_case(24, 149, 111, 32, 32, "fan", "exact", fan=8)
    with pytest.raises(_abi.CfsdError):
        flat_dx(c, False)


# ------------------------------------------------------------------ the xyz output conv, vertex-major
def out_flat(c, x_bf16, with_dx, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    x = c.dev("x", x_bf16, True)
    ey = c.dev("elu_y", x_bf16, True)
    dx = nan_out((batch, vsrc, cin), x_bf16, True) if with_dx else None
    dw, db = nan_out((cout, seq * cin)), nan_out((cout,))
    ws = nan_ws(ops.spiral_conv_bwd_workspace(batch, vsrc, rows, seq, cin, cout))
    args = (x, c.d["idx"], c.dev("dpre", vm=True), c.flat, c.d["w"])
    if not deferred:
        r = ops.spiral_conv_bwd_out_flat(*args, dw, db, dx=dx, elu_y=ey if with_dx else None, workspace=ws)
        assert r is dx
    else:
        r = ops.spiral_conv_bwd_out_flat(*args, None, None, dx=dx, elu_y=ey if with_dx else None, workspace=ws)
        item = r[1] if with_dx else r
        assert isinstance(item, ops.DeferredDw)
        ops.dw_reduce_batch([(item, dw, db)])
    return dx, dw, db


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("x_bf16", [False, True], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("fan", [12, 16, 20])
@pytest.mark.parametrize("batch,vsrc", [(16, 149), (32, 3644)])
def test_output_conv_fused_backward_flat(batch, vsrc, fan, x_bf16, mode):
    """``ops.spiral_conv_bwd_out_flat`` (conv_bwd_out_vm<float or bf16_t, width>), with and without dx."""
    c = make_conv_case(batch, vsrc, vsrc, 32, 3, "fan", mode, fan=fan, bf16=("x", "elu_y") if x_bf16 else (),
                       parts=("dx", "dw"))
    cd = c.on_device()
    assert c.flat[1] == fan and ops.spiral_conv_has_shape(ops.CONV_BWD_FUSED, SEQ, 32, 3)
    tag = "out flat " + ("bf16" if x_bf16 else "fp32")
    dx, dw, db = out_flat(c, x_bf16, True, False)
    ref, tol = cd.with_elu_grad(cd.dx, cd.tol_dx())
    compare(tag + " dx*elu'", dx, ref, tol, c.shape, c.exact)
    compare(tag + " dw", dw, cd.dw, cd.tol_dw(), c.shape, c.exact)
    compare(tag + " db", db, cd.db, cd.tol_db(), c.shape, c.exact)
    assert_exact_zeros(c, dx, True)
    for deferred in (True, False):
        dx2, dw2, db2 = out_flat(c, x_bf16, True, deferred)
        assert same(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)
    _, dw3, db3 = out_flat(c, x_bf16, False, False)   # no dx: the same slabs
    assert torch.equal(dw3, dw) and torch.equal(db3, db)


def test_output_conv_fused_backward_flat_refusals():
    c = make_conv_case(16, 149, 111, 32, 3, "fan", "exact", fan=8)   # rows != vsrc
    with pytest.raises(_abi.CfsdError):
        out_flat(c, False, True, False)
    c = make_conv_case(24, 149, 149, 32, 3, "fan", "exact", fan=12)  # batch % 16
    with pytest.raises(_abi.CfsdError):
        out_flat(c, False, True, False)


OUT_GEOMS = [(8, 37, 37, "head_edge"), (24, 2731, 2731, "hubs"), (24, 2731, 2731, "head_edge")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("x_bf16", [False, True], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("cout", [1, 2, 3])
@pytest.mark.parametrize("batch,vsrc,rows,table", OUT_GEOMS)
def test_output_conv_forward_vertex_major(batch, vsrc, rows, table, cout, x_bf16, mode):
    """``ops.spiral_conv_fwd_x``, 32 -> 1 / 2 / 3 with a vertex-major x of either type, batch % 8 == 0
    (conv_fwd_out_vm), y in both layouts, both activations."""
    c = make_conv_case(batch, vsrc, rows, 32, cout, table, mode, bf16=("x",) if x_bf16 else (), parts=("fwd",))
    cd = c.on_device()
    for yvm in (True, False):
        for act in (ACT_NONE, ACT_ELU):
            y = fwd_x(c, act, True, yvm, x_bf16=x_bf16)
            check_fwd(c, cd, y, act, "fwd_x out vm " + ("bf16" if x_bf16 else "fp32"))
            assert same(fwd_x(c, act, True, yvm, x_bf16=x_bf16), y)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("batch,vsrc,rows,table", [(8, 37, 37, "head_edge"), (24, 2731, 2731, "head_edge"),
                                                   (3, 2731, 2731, "hubs"), (16, 2731, 2731, "hubs"),
                                                   (16, 2731, 683, "random")])
def test_input_conv_mixed_outputs_and_gradients(batch, vsrc, rows, table, cout, mode):
    """The xyz input conv, 3 -> 32 / 64: ``ops.spiral_conv_fwd_x`` with y vertex-major and / or bf16
    (fwd_xyz_in) and ``ops.spiral_conv_bwd_weight_x`` with dpre bf16 and / or vertex-major (dw_xyz_in)."""
    c = make_conv_case(batch, vsrc, rows, 3, cout, table, mode, bf16=("dpre",), parts=("fwd", "dw"))
    cd = c.on_device()
    for yvm in (False, True):
        for y_bf16 in (False, True):
            for act in (ACT_NONE, ACT_ELU):
                y = fwd_x(c, act, False, yvm, y_bf16=y_bf16)
                check_fwd(c, cd, y, act, "fwd_x xyz in")
                assert same(fwd_x(c, act, False, yvm, y_bf16=y_bf16), y)
    for dpvm in (False, True):
        for dp_bf16 in (False, True):
            dw_case(c, cd, False, dpvm, "dw_x xyz in", dp_bf16=dp_bf16)


# ------------------------------------------------------------------ cfsd_spiral_conv_bwd_x with bf16 operands
def bwd_x(c, x_bf16, vm, with_dx, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    x, ey = c.dev("x", x_bf16, vm), c.dev("elu_y", x_bf16, vm)
    dx = nan_out((batch, vsrc, cin), x_bf16, vm) if with_dx else None
    dw, db = nan_out((cout, seq * cin)), nan_out((cout,))
    ws = nan_ws(ops.spiral_conv_bwd_workspace(batch, vsrc, rows, seq, cin, cout))
    args = (x, c.d["idx"], c.d["dpre"], c.inv, c.d["w"])
    if not deferred:
        r = ops.spiral_conv_bwd_x(*args, dw, db, dx=dx, elu_y=ey if with_dx else None, workspace=ws)
        assert r is dx
    else:
        r = ops.spiral_conv_bwd_x(*args, None, None, dx=dx, elu_y=ey if with_dx else None, workspace=ws)
        item = r[1] if with_dx else r
        assert isinstance(item, ops.DeferredDw)
        ops.dw_reduce_batch([(item, dw, db)])
    return dx, dw, db


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", [(32, 3), (64, 3), (32, 1), (64, 2)])
@pytest.mark.parametrize("batch,vsrc,rows,table", [(3, 2731, 2731, "hubs"), (3, 2731, 2731, "head_edge"),
                                                   (16, 2731, 2731, "hubs"), (16, 2731, 2731, "head_edge")])
def test_fused_small_output_backward_bf16_operands(batch, vsrc, rows, table, cin, cout, mode):
    """``ops.spiral_conv_bwd_x`` (bwd_fused_small) with x / elu_y / dx in bf16, both layouts."""
    c = make_conv_case(batch, vsrc, rows, cin, cout, table, mode, bf16=("x", "elu_y"), parts=("dx", "dw"))
    cd = c.on_device()
    gm = gamma(cd.n_dx_inverse())
    ref, tol = cd.with_elu_grad(cd.dx, gm * cd.dx_abs)
    for vm in (False, True):
        tag = "bwd_x bf16 " + ("vm" if vm else "bm")
        dx, dw, db = bwd_x(c, True, vm, True, False)
        compare(tag + " dx*elu'", dx, ref, tol, c.shape, c.exact)
        compare(tag + " dw", dw, cd.dw, cd.tol_dw(), c.shape, c.exact)
        compare(tag + " db", db, cd.db, cd.tol_db(), c.shape, c.exact)
        assert_exact_zeros(c, dx, True)
        for deferred in (True, False):
            dx2, dw2, db2 = bwd_x(c, True, vm, True, deferred)
            assert same(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)
        _, dw3, db3 = bwd_x(c, True, vm, False, False)
        compare(tag + " dw (no dx)", dw3, cd.dw, cd.tol_dw(), c.shape, c.exact)
        compare(tag + " db (no dx)", db3, cd.db, cd.tol_db(), c.shape, c.exact)
