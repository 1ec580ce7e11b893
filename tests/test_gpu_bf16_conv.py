"""The bf16 MFMA SpiralConv kernels (``spiral_conv_bf16.hip``: conv_fwd_b16 / conv_dx_b16 / conv_dw_b16;
``spiral_conv_vm16.hip``: conv_fwd_vm16 / conv_dx_vm16 / conv_dx_flat_vm16 / conv_dw_vm16 and the two pairs)
through ``cfsd_spiral_conv_fwd_x`` / ``_bwd_data_x`` / ``_bwd_data_flat`` / ``_bwd_weight_x`` /
``_bwd_flat_pair_bf16`` / ``_bwd_rowsub_pair_bf16`` / ``_bwd_data_rowsub`` on the synthetic spiral tables of
``tests/golden/spiral_tables.py`` against the fp64 restatement of ``conv_cases.Case``.  The method (exact and
randn input modes, NaN pre-fill, second call, deferred == immediate, exact zeros) is that of
``test_gpu_vertex_major_conv``; the step-level and layout-agreement tests stay in ``test_gpu_bf16.py``.

Exact mode.  x, w, b, elu_y from the dyadic sets, dpre from {-1, 0, 1}: the inverse-table dx kernels round
the per-slot list sum A_s[u, o] to bf16 before the MFMA, and a sum of signs is an integer that bf16 holds up to
256 -- ``make_conv_case(..., inverse_bf16=True)`` asserts on the CPU that every A_s of the case round-trips
through bf16 (and the 2^24 conditions), so fp32 results must EQUAL the restatement and bf16 results the
restatement rounded to nearest even (``f2bf`` is ``(__bf16)f``).  This is the mode that sees a lost list entry
on a hub: under a rounding bound, 2^-8 * sum|terms| of a 1365-row list is larger than a whole term.

randn mode: the rounding model.  x, w, elu_y (and dpre, see below) are rounded to bf16 BEFORE the reference sees
them (``Case(bf16=...)``); the bias stays fp32 (the kernels read it as fp32).  A product of two bf16 values is
exact in fp32; accumulation is fp32 with unit roundoff ``conv_cases.UM`` per MFMA-accumulated step (2^-24
assumed; DESIGN.md records what the hardware needed).  Per kernel, from its code:

    conv_fwd_b16, conv_fwd_vm16      acc over 9 cin products (MFMA chain), + bias, ELU, store: n = 9 cin + 1; a
                                     bf16 y adds 2^-8 (|ref| + tol).  conv_fwd_vm16 runs the MFMA transposed:
                                     same count.
    conv_dx_b16, conv_dx_vm16        per slot: the list's dpre rows summed in fp32 in list order (head rows
                                     (r0 + r1) + r2, + r3, the CSR tail walk: E_s - 1 adds; a bf16 dpre is
                                     widened exactly), ONE rounding of A_s to bf16 (pack_bf2), then the MFMA
                                     chain over cout products for each of the S non-empty slots:
                                     tol = (gamma_n + 2^-8 (1 + gamma_n)) dx_abs, n = max_s E_s - 1 + cout S,
                                     dx_abs = sum |dpre| |w|; ELU' one more u; the bf16 dx 2^-8 (|ref| + tol).
                                     With an fp32 dpre the list sum is over the UNROUNDED values: the reference
                                     of that variant uses a second, unrounded dpre.
    conv_dx_flat_vm16                one MFMA per list entry: an fp32 dpre row is rounded to bf16 PER ENTRY when
                                     the B fragment is packed (pack_bf2 in dx_flat_vm16_body), so the reference
                                     is on the rounded dpre for either storage; n = E(u) cout.
    conv_dw_b16, conv_dw_vm16        dpre is an MFMA operand: an fp32 dpre is rounded per element by ld8bf
                                     (conv_dw_b16's load_tile) / pack_bf2 (dw_vm16_body's load_unit), and db sums
                                     the ROUNDED values (bf2f of the staged tile / of the A fragment): reference
                                     on the rounded dpre; n = batch * rows.
    conv_dx_flat_vm32<.., bf16_t>    fp32 dpre and fp32 w, fp32 MFMA chain (u = 2^-24), one rounding of the
                                     result: n = E(u) cout, then 2^-8 (|ref| + tol).  Behind
                                     cfsd_spiral_conv_bwd_rowsub_pair_bf16 and cfsd_spiral_conv_bwd_data_rowsub.

Which kernel a case reaches (bf::launch_fwd / launch_dx / launch_dw): vertex-major x (dx and dpre for the data
gradient) with batch % 16 == 0 and cin == 32 takes the vm16 kernel, everything else conv_*_b16 with its layout
flags; the weight gradient takes conv_dw_vm16 for 32 -> 32, x vertex-major, batch % 16 == 0 and dpre either
bf16 vertex-major or fp32 batch-major (dw_vm16_ok).  ``kernels_of`` restates that; the slab code is the
library's (``cfsd_spiral_conv_bwd_weight_x_slabs`` == CFSD_DW_BF16).

    case (batch x vsrc, rows = vsrc unless given)   what it is there for
    ---------------------------------------------   ----------------------------------------------------------
    1 x 37 (head_edge)                              M % 16 = 5 and M % 32 = 5: one full and one partial tile
    3 x 2731            M = 8193                    M % 16 = 1, M % 32 = 1; batch-major kernels only
    16 x 149, 48 x 149                              vm16 kernels with one and three mesh groups per vertex
    16 x 2731                                       vm16 kernels, many tiles per wave
    16 x 2049           M = 32784, 1025 tiles       bf::dw_slabs: (2 * 1025 + 7) / 8 = 257 (32 -> 32) and
                                                    (1025 + 3) / 4 = 257 (64 -> 64) slabs, capped at 256
    16 x 4097 (hubs)                                lists of 683 rows on a hub key: the CSR tail walk
    16 x 2731 rows 683, 16 x 911 rows 2733          Enblock form / three rows per source vertex, also with
                                                    ``random`` and ``one_vertex_rows``
    flat: 16 x 149, 16 x 3644 (rows 111 / 2733      conv_dx_flat_vm16<32, 32 | 64, float | bf16_t, 8..20>,
          for width 8)                              conv_bwd_vm16_pair<8..20>
    row subset: 16 x 149 rows 37, 16 x 3644         conv_bwd_rowsub16_pair<4..16>, conv_dx_flat_vm32<.., bf16_t>
          rows 911

Measured on an MI355X (largest err / bound of the randn mode; DESIGN.md section 15 has the full table), with
u = 2^-24 on the MFMA chains -- nothing had to move to 2^-23: conv_dw_b16 0.045, conv_dw_vm16 and the pairs' dW below
0.001 (fp32 results of bf16 MFMA chains); conv_dx_b16 0.507 (bf16 dpre) / 0.601 (fp32 dpre), conv_dx_vm16 0.493 /
0.591 (the A_s rounding and the store); every other bf16-stored result 0.98 .. 1.00 -- the store's own half unit
in the last place against 2^-8 |ref| (bf16's unit roundoff: 2^-9 gave 1.99 at bit-exact rounding).  Exact mode: ELU
branch at most 0.49 of 2^-23.

Not covered, with the reason:
  * conv_dx_vm16 / conv_fwd_vm16 with cin = 64: vm16_ok requires cin == 32; such a layer takes conv_*_b16 with the
    vertex-major flags (covered).
  * conv_dw_vm16<float> with a vertex-major dpre and conv_dw_vm16<bf16_t> with a batch-major one: dw_vm16_ok
    routes both to conv_dw_b16 (covered there).
  * conv_bwd_rowsub16_pair<20> / conv_bwd_vm16_pair<4>: not instantiated (refusal asserted).
"""
import pytest
import torch

import exact_values as X
from conv_cases import (ACT_ELU, ACT_NONE, CHUNK, SEQ, assert_exact_zeros, compare, compare_elu_fwd, host_threads,
                        make_conv_case, nan_out, nan_ws, put, same)
from craniofacialsd_vae_amd import _abi, ops

pytestmark = pytest.mark.gpu

MODES = ("exact", "randn")
ALL_BF16 = ("x", "w", "dpre", "elu_y")
BOTH = ("hubs", "head_edge")
SHAPES = [(32, 32), (32, 64), (64, 32), (64, 64)]
LAYOUTS = [(False, False), (True, True), (True, False), (False, True)]


def kernels_of(batch, cin, cout):
    """Which (xvm, second operand vm) pairs reach the vm16 kernels (module docstring)."""
    vm16 = batch % 16 == 0 and cin == 32
    return {"fwd": lambda xvm: "vm16" if vm16 and xvm else "b16",
            "dx": lambda dpvm, dxvm: "vm16" if vm16 and dpvm and dxvm else "b16",
            "dw": lambda xvm, dpvm, dp_bf16: "vm16" if (vm16 and cout == 32 and xvm and dpvm == dp_bf16) else "b16"}


# ------------------------------------------------------------------ forward, inverse-table dx, dW
def fwd_b(c, act, xvm, yvm, y_bf16):
    batch, vsrc, rows, seq, cin, cout = c.shape
    y = nan_out((batch, rows, cout), y_bf16, yvm)
    ops.spiral_conv_fwd_x(c.dev("x", True, xvm), c.d["idx"], c.d["w"], c.dev("w", True), c.d["b"], act, y)
    return y


def dx_b(c, dpre_dev, dxvm, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ey = c.dev("elu_y", True, dxvm) if elu else None
    return ops.spiral_conv_bwd_data_x(dpre_dev, c.inv, c.dev("w", True), vsrc, elu_y=ey,
                                      out=nan_out((batch, vsrc, cin), True, dxvm))


def dw_b(c, xvm, dpvm, dp_bf16, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    need = ops.spiral_conv_bwd_weight_x_workspace(batch, rows, seq, cin, cout)
    assert need > 0
    x, dp = c.dev("x", True, xvm), c.dev("dpre", dp_bf16, dpvm)
    dw, db = nan_out((cout, seq * cin)), nan_out((cout,))
    if not deferred:
        assert ops.spiral_conv_bwd_weight_x(x, c.d["idx"], dp, dw, db, nan_ws(need)) is None
    else:
        item = ops.spiral_conv_bwd_weight_x(x, c.d["idx"], dp, None, None, nan_ws(need))
        assert isinstance(item, ops.DeferredDw)
        ops.dw_reduce_batch([(item, dw, db)])
    return dw, db


MFMA_CASES = [
    (1, 37, 37, ("head_edge",), SHAPES),
    (3, 2731, 2731, BOTH, SHAPES),
    (16, 149, 149, ("head_edge",), SHAPES),
    (48, 149, 149, ("head_edge",), SHAPES),
    (16, 2731, 2731, BOTH, SHAPES),
    (16, 2049, 2049, ("hubs",), [(32, 32), (64, 64)]),
    (16, 4097, 4097, BOTH, SHAPES),
    (16, 2731, 683, BOTH + ("random", "one_vertex_rows"), SHAPES),
    (16, 911, 2733, BOTH + ("random", "one_vertex_rows"), SHAPES),
]
MFMA_PARAMS = [pytest.param(b, v, r, t, ci, co, m, id=f"{b}x{v}-rows{r}-{ci}to{co}-{t}-{m}")
               for b, v, r, tables, shapes in MFMA_CASES for t in tables for ci, co in shapes for m in MODES]


@pytest.mark.parametrize("batch,vsrc,rows,table,cin,cout,mode", MFMA_PARAMS)
def test_bf16_mfma_kernels(batch, vsrc, rows, table, cin, cout, mode):
    """Forward (y fp32 / bf16, both activations), inverse-table dx (dpre fp32 / bf16, with and without ELU')
    and dW / db (dpre fp32 / bf16) of one bf16 conv in all four layout pairs."""
    c = make_conv_case(batch, vsrc, rows, cin, cout, table, mode, dpre_values=X.SIGNS, bf16=ALL_BF16,
                       inverse_bf16=True)
    cd = c.on_device()
    which = kernels_of(batch, cin, cout)
    layouts = LAYOUTS if batch > 1 else LAYOUTS[:1]
    if (batch, rows) == (16, 2049):   # above the slab cap of bf::dw_slabs
        n_el = cout * SEQ * cin + cout
        assert ops.spiral_conv_bwd_weight_x_workspace(batch, rows, SEQ, cin, cout) == 256 * n_el * 4
        tiles = (batch * rows + 31) // 32
        assert ((2 * tiles + 7) // 8 if cout == 32 else (tiles + 3) // 4) > 256
    # ---- forward
    for xvm, yvm in layouts:
        for y_bf16 in (False, True):
            for act in (ACT_NONE, ACT_ELU):
                y = fwd_b(c, act, xvm, yvm, y_bf16)
                tag = f"fwd {which['fwd'](xvm)}"
                if act == ACT_NONE:
                    compare(tag, y, cd.pre, cd.tol_fwd_b16(), c.shape, c.exact)
                else:
                    compare_elu_fwd(tag + "+elu", y, cd.pre, cd.tol_fwd_b16(), c.shape, c.exact)
                assert same(fwd_b(c, act, xvm, yvm, y_bf16), y)
    # ---- inverse-table dx: an fp32 dpre is summed unrounded (randn mode: a second dpre and its dx)
    if c.exact:
        dp32, dx32, dx32_abs = c.dpre, cd.dx, cd.dx_abs
    else:
        g = torch.Generator().manual_seed(batch + vsrc + rows + cin + cout)
        dp32 = torch.randn(batch, rows, cout, generator=g)
        with host_threads():
            dx32, dx32_abs = (t.to(cd.dx.device) for t in X.restate_dx(c.idx, c.w, dp32, vsrc, CHUNK))
    for dp_bf16 in (True, False):
        ref0, abs0 = (cd.dx, cd.dx_abs) if dp_bf16 else (dx32, dx32_abs)
        for dpvm, dxvm in layouts:
            dpre_dev = c.dev("dpre", True, dpvm) if dp_bf16 else put(dp32, False, dpvm)
            for elu in (False, True):
                tol = cd.tol_dx_inverse_b16(abs0)
                ref, tol = cd.with_elu_grad(ref0, tol) if elu else (ref0, tol)
                dx = dx_b(c, dpre_dev, dxvm, elu)
                tag = f"dx {which['dx'](dpvm, dxvm)} dpre {'bf16' if dp_bf16 else 'fp32'}" + ("*elu'" if elu else "")
                compare(tag, dx, ref, tol, c.shape, c.exact)
                assert_exact_zeros(c, dx, elu)
                assert same(dx_b(c, dpre_dev, dxvm, elu), dx)
    # ---- dW / db
    lib = _abi.lib()
    for dp_bf16 in (True, False):
        for xvm, dpvm in layouts:
            assert lib.cfsd_spiral_conv_bwd_weight_x_slabs(ops._st(c.dev("x", True, xvm)),
                                                           ops._st(c.dev("dpre", dp_bf16, dpvm)), batch, cin,
                                                           cout) == ops.DW_BF16
            tag = f"dw {which['dw'](xvm, dpvm, dp_bf16)} dpre {'bf16' if dp_bf16 else 'fp32'}"
            dw, db = dw_b(c, xvm, dpvm, dp_bf16, False)
            compare(tag + " dw", dw, cd.dw, cd.tol_dw_b16(), c.shape, c.exact)
            compare(tag + " db", db, cd.db, cd.tol_db_b16(), c.shape, c.exact)
            for deferred in (True, False):
                dw2, db2 = dw_b(c, xvm, dpvm, dp_bf16, deferred)
                assert torch.equal(dw2, dw) and torch.equal(db2, db), (tag, deferred)


def test_bf16_entry_points_refuse_what_they_have_no_kernel_for():
    c = make_conv_case(16, 149, 149, 32, 32, "head_edge", "exact", dpre_values=X.SIGNS, bf16=ALL_BF16)
    batch, vsrc, rows, seq, cin, cout = c.shape
    with pytest.raises(ValueError):   # dx must be bf16
        ops.spiral_conv_bwd_data_x(c.dev("dpre", True), c.inv, c.dev("w", True), vsrc, out=nan_out((batch, vsrc, cin)))
    with pytest.raises(_abi.CfsdError):   # a bf16 x needs the bf16 weight shadow
        ops.spiral_conv_fwd_x(c.dev("x", True), c.d["idx"], c.d["w"], None, c.d["b"], ACT_NONE,
                              nan_out((batch, rows, cout)))
    with pytest.raises(_abi.CfsdError):   # fp32 x with a bf16 dpre
        ops.spiral_conv_bwd_weight_x(c.dev("x"), c.d["idx"], c.dev("dpre", True), nan_out((cout, seq * cin)),
                                     nan_out((cout,)), nan_ws(1 << 22))


# ------------------------------------------------------------------ flat-list dx and the full-table pair
def flat_dx_b(c, dp_bf16, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ey = c.dev("elu_y", True, True) if elu else None
    return ops.spiral_conv_bwd_data_flat(c.dev("dpre", dp_bf16, True), c.flat, c.dev("w", True), vsrc, elu_y=ey,
                                         out=nan_out((batch, vsrc, cin), True, True))


def flat_pair_b(c, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ws = nan_ws(ops.spiral_conv_bwd_weight_x_workspace(batch, rows, seq, cin, cout))
    dx, dw, db = nan_out((batch, vsrc, cin), True, True), nan_out((cout, seq * cin)), nan_out((cout,))
    ey = c.dev("elu_y", True, True) if elu else None
    item = ops.spiral_conv_bwd_flat_pair_bf16(c.dev("x", True, True), c.d["idx"], c.dev("dpre", True, True), c.flat,
                                              c.dev("w", True), dx, elu_y=ey, workspace=ws)
    assert isinstance(item, ops.DeferredDw)
    ops.dw_reduce_batch([(item, dw, db)])
    return dx, dw, db


FLAT_CASES = [(16, 149, 149, (12, 16, 20)), (16, 149, 111, (8,)), (16, 3644, 3644, (12, 16, 20)), (16, 3644, 2733, (8,))]
FLAT_PARAMS = [pytest.param(b, v, r, f, co, m, id=f"{b}x{v}-rows{r}-32to{co}-fan{f}-{m}")
               for b, v, r, fans in FLAT_CASES for f in fans for co in (32, 64) for m in MODES]


@pytest.mark.parametrize("batch,vsrc,rows,fan,cout,mode", FLAT_PARAMS)
def test_flat_list_data_gradient_and_pair_bf16(batch, vsrc, rows, fan, cout, mode):
    """``ops.spiral_conv_bwd_data_flat`` with bf16 operands (conv_dx_flat_vm16, dpre fp32 / bf16) and, for
    32 -> 32, ``ops.spiral_conv_bwd_flat_pair_bf16`` (conv_bwd_vm16_pair: the same dx and the conv_dw_vm16
    slabs, always deferred)."""
    c = make_conv_case(batch, vsrc, rows, 32, cout, "fan", mode, fan=fan, dpre_values=X.SIGNS, bf16=ALL_BF16,
                       parts=("dx", "dw") if cout == 32 else ("dx",))
    cd = c.on_device()
    assert c.flat[1] == fan
    for elu in (False, True):
        ref, tol = cd.with_elu_grad(cd.dx, cd.tol_dx_flat_b16()) if elu else (cd.dx, cd.tol_dx_flat_b16())
        for dp_bf16 in (True, False):
            dx = flat_dx_b(c, dp_bf16, elu)
            assert ops.is_vm(dx)
            compare(f"dx flat vm16 dpre {'bf16' if dp_bf16 else 'fp32'}" + ("*elu'" if elu else ""), dx, ref, tol,
                    c.shape, c.exact)
            assert_exact_zeros(c, dx, elu)
            assert same(flat_dx_b(c, dp_bf16, elu), dx)
        if cout == 32:
            dx, dw, db = flat_pair_b(c, elu)
            compare("pair vm16 dx" + ("*elu'" if elu else ""), dx, ref, tol, c.shape, c.exact)
            compare("pair vm16 dw", dw, cd.dw, cd.tol_dw_b16(), c.shape, c.exact)
            compare("pair vm16 db", db, cd.db, cd.tol_db_b16(), c.shape, c.exact)
            assert_exact_zeros(c, dx, elu)
            dx2, dw2, db2 = flat_pair_b(c, elu)
            assert same(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)


# ------------------------------------------------------------------ the Enblock pair (row subset)
def rowsub_pair_b(c, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ws = nan_ws(ops.spiral_conv_bwd_weight_x_workspace(batch, rows, seq, cin, cout))
    dx, dw, db = nan_out((batch, vsrc, cin), True, True), nan_out((cout, seq * cin)), nan_out((cout,))
    ey = c.dev("elu_y", True, True) if elu else None
    item = ops.spiral_conv_bwd_rowsub_pair_bf16(c.dev("x", True, True), c.d["idx"], c.d["dpre"], c.flat, c.d["w"], dx,
                                                elu_y=ey, workspace=ws)
    assert isinstance(item, ops.DeferredDw)
    ops.dw_reduce_batch([(item, dw, db)])
    return dx, dw, db


def rowsub_data_b(c, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ws = nan_ws(ops.spiral_conv_bwd_data_rowsub_workspace(batch, rows, seq, cin))
    ey = c.dev("elu_y", True, True) if elu else None
    return ops.spiral_conv_bwd_data_rowsub(c.d["dpre"], c.flat, c.d["w"], vsrc, elu_y=ey,
                                           out=nan_out((batch, vsrc, cin), True, True), workspace=ws)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fan", [4, 8, 12, 16])
@pytest.mark.parametrize("batch,vsrc,rows", [(16, 149, 37), (16, 3644, 911)])
def test_row_subset_pair_bf16(batch, vsrc, rows, fan, mode):
    """``ops.spiral_conv_bwd_rowsub_pair_bf16`` (conv_bwd_rowsub16_pair: fp32-product flat dx rounded once to
    bf16, and the conv_dw_vm16<float> slabs) and the dx alone through ``ops.spiral_conv_bwd_data_rowsub``
    (conv_dx_flat_vm32<32, 32, width, bf16_t>).  dpre fp32 batch-major holding bf16-exact values (the dW half
    rounds it per element), w fp32 unrounded."""
    c = make_conv_case(batch, vsrc, rows, 32, 32, "fan", mode, fan=fan, dpre_values=X.SIGNS,
                       bf16=("x", "dpre", "elu_y"), parts=("dx", "dw"))
    cd = c.on_device()
    assert c.flat[1] == fan
    for elu in (False, True):
        ref, tol = cd.with_elu_grad(cd.dx, cd.tol_dx()) if elu else (cd.dx, cd.tol_dx())
        dx, dw, db = rowsub_pair_b(c, elu)
        compare("rowsub pair bf16 dx" + ("*elu'" if elu else ""), dx, ref, tol, c.shape, c.exact)
        compare("rowsub pair bf16 dw", dw, cd.dw, cd.tol_dw_b16(), c.shape, c.exact)
        compare("rowsub pair bf16 db", db, cd.db, cd.tol_db_b16(), c.shape, c.exact)
        assert_exact_zeros(c, dx, elu)
        dx2, dw2, db2 = rowsub_pair_b(c, elu)
        assert same(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)
        dxd = rowsub_data_b(c, elu)
        compare("rowsub data bf16 dx" + ("*elu'" if elu else ""), dxd, ref, tol, c.shape, c.exact)
        assert_exact_zeros(c, dxd, elu)
        assert same(rowsub_data_b(c, elu), dxd)


def test_pairs_refuse_other_widths_and_batches():
    """Width 4 for the full-table pair, width 20 for the row-subset pair, batch 24 for either."""
    c = make_conv_case(16, 149, 37, 32, 32, "fan", "exact", fan=4, dpre_values=X.SIGNS, bf16=("x", "dpre", "elu_y"))
    with pytest.raises(_abi.CfsdError):
        flat_pair_b(c, False)
    c = make_conv_case(16, 149, 149, 32, 32, "fan", "exact", fan=20, dpre_values=X.SIGNS, bf16=("x", "dpre", "elu_y"))
    with pytest.raises(_abi.CfsdError):
        rowsub_pair_b(c, False)
    c = make_conv_case(24, 149, 111, 32, 32, "fan", "exact", fan=8, dpre_values=X.SIGNS, bf16=("x", "dpre", "elu_y"))
    for run in (flat_pair_b, rowsub_pair_b, lambda cc, e: flat_dx_b(cc, True, e)):
        with pytest.raises(_abi.CfsdError):
            run(c, False)
