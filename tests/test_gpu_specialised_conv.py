"""The specialised spiral-length-9 SpiralConv kernels (``cfsd_spiral_conv_fwd`` / ``_bwd_data`` /
``_bwd_weight`` / ``_bwd`` / ``_fwd_up`` / ``_bwd_rowsub`` / ``_bwd_data_rowsub``, fp32 batch-major) on
the synthetic spiral tables of ``tests/golden/spiral_tables.py`` against the fp64 restatement of
``conv_cases.Case``, at the sizes where the dispatch of ``spiral_conv.hip`` changes kernel.

Bounds (derived, per element; ``test_gpu_general_conv``'s docstring has the model: a sum of n terms
in any order has |err| <= gamma_n * sum|terms|, gamma_n = n u / (1 - n u), u = 2^-24; adding an exact
0 -- an empty list, an absent row read through an out-of-range buffer offset, the 0-weighted clamped
row of a partial tile -- rounds nothing).  Re-derived per kernel family from its code:

    forward   n = 9 cin + 1.  One fmaf chain over 9 cin products and the bias (conv_fwd_lat,
              conv_fwd_mfma with 9 slots, conv_fwd_in_*, conv_fwd_out_small), or per-slot-group
              chains of cin (coarse conv_fwd_ks / conv_fwd_pt: 9 partials summed in LDS) or 3 cin
              (conv_fwd_mfma with 3 slots + conv_combine) products, then 2 to 8 adds and the bias:
              every term passes at most cin + 9 <= 9 cin + 1 roundings (cin >= 1).
    dx        n(u) = max_s E_s - 1 + cout * S, for E_s rows on key (u, s) and S non-empty slots -- never
              more than the general family's entries(u) * cout (E_s - 1 <= E - S, and E >= S), and far
              less on a hub.  Per slot the list's dpre rows are added first (E_s - 1 adds: the head
              rows (r0 + r1) + r2, then + r3, then the tail walk in list order), then one fmaf per
              output channel of every non-empty slot (conv_dx_mfma, conv_dx_out_small, the fused
              conv_bwd_out_mfma: one chain of cout S; conv_dx_lat: two accumulators of cout S / 2 and
              their sum; conv_dx_ks and conv_dx_mfma with 3 slots + conv_combine: chains of cout or
              3 cout, then at most S - 1 non-zero partial adds, and cout + S - 1 <= cout S).  The
              shorter count is used because the general one cannot see a lost list entry on a hub:
              with E = 2458 entries and cout = 32, gamma_{E cout} * sum|terms| is about 240 while a whole
              term is below 40 (measured with one tail walk starting an entry late: the ``hubs`` case
              passed under E cout and fails under this count).  No entries: n = 0, exactly 0.
    dW / db   n = batch * rows.  dW[o, s cin + c] sums one product per (mesh, row); row chunks,
              per-workgroup slabs and the slab reduce (immediate or cfsd_dw_reduce_batch) are one
              summation tree over those terms.  The fused small-output kernel forms its terms in
              SOURCE-row space, T_s[u, o] . x[u, c] with T_s the list sum: E_s - 1 adds, then a
              chain over batch * vsrc tile rows of which only the non-empty keys add a non-zero --
              no more operations with a non-zero operand than batch * rows in all, so the same n.
    row subset dx: dG[r, s cin + c] = sum_o dpre[r, o] w[o, .] on two accumulators (cout / 2 + 1
              roundings), then the flat-list gather adds E(u) rows: cout / 2 + E <= E cout.  At
              batch 16, 32 -> 32, the flat-list MFMA kernel (vm32::conv_bwd_flat_pair /
              conv_dx_flat_vm32) chains cout fmafs per entry into one accumulator: E cout.
    fused up  Pool(up) first: up[r] = v0 x[c0] + v1 x[c1] + v2 x[c2] (3 roundings, bound gamma_3 on
              the up-sampled row itself), then the coarse forward on it: n = 9 cin + 1 + 3, with
              sum|terms| = |w| . (|v| . |x|) + |b|.
    ELU / ELU': one more u, as in test_gpu_general_conv.  elu_y holds entries that are exactly -1
              (g = 0) and exactly 0; where g = 0 or the vertex is in no spiral dx must be exactly 0.

No chain is longer than the general family's: its n are used for the forward, dW / db and the
flat-list (row-subset) dx, and the shorter per-vertex count above for the inverse-table dx.

Every output and every workspace is pre-filled with NaN (an element left unwritten, or a reduce
reading a slab nobody wrote, then shows: ``chk`` refuses a non-finite result before comparing).
Every case also asserts that a second call is bit-identical and that the deferred weight gradient
(``dw is db is None``, then ``ops.dw_reduce_batch``) equals the immediate one bit for bit.

Which branch a case takes is argued from the constants of ``spiral_conv.hip`` /
``spiral_conv_coarse.hip`` restated below, and from the library's own queries where it has one
(``spiral_conv_bwd_paired``, ``spiral_conv_fwd_up_supported``, ``spiral_conv_has_shape``).  M is
batch * rows for forward and dW and batch * vsrc for dx; batch 3 and odd vertex counts make the last
tile of every tiling (16, 32, 64 rows) partial.

    case (batch x vsrc, rows = vsrc unless given)   constant it sits next to     branch it is meant to take
    ---------------------------------------------   --------------------------   ------------------------------------
    1 x 37                                          --                           as 3 x 2729: three 16-row tiles, the last one partial
    3 x 2729   M = 8187                             kMaxTilesFew * 16 = 8192     fwd conv_fwd_ks<.,.,9,1,0>; dx conv_dx_ks<.,.,9,2>;
                                                                                 bwd conv_bwd_ks_pair<.,.,9,2> ("ks"); dW conv_dw_lat,
                                                                                 64 -> 64 with lat_geom's own chunk sizing
    3 x 2731   M = 8193                             the same, other side         fwd conv_fwd_pt<.,.,0>; dx conv_dx_lat<32,.,1> /
                                                                                 <64,.,2>; bwd conv_bwd_lat_pair<32,32,1> / <64,32,2>
                                                                                 ("lat"), cout 64 two launches ("two")
    3 x 8191   M = 24573                            coarse::kMaxRows = 24576     fwd conv_fwd_pt (last size on it)
    3 x 8193   M = 24579                            the same, other side         fwd conv_fwd_lat<32,32,.,1> / <32,64,.,1> / <64,64,.,2>;
                                                                                 64 -> 32: conv_fwd_mfma<64,32,.,3> + conv_combine
                                                                                 (pick_spg: 400 <= 769 tiles < 2048)
    3 x 8193, 64 -> 32 forward, workspace too       pick_spg's loop              conv_fwd_mfma<64,32,.,9>, no combine
              small for 3 slot groups
    3 x 10923  M = 32769                            dx_lat_ctw: 32768            32 -> 32 dx conv_dx_lat<32,32,2>, bwd conv_bwd_lat_pair<32,32,2>
    3 x 21845  M = 65535                            kLatMaxRows = 65536          last size of conv_fwd_lat / conv_dx_lat / conv_dw_lat and the
                                                                                 lat pair; 64 -> 32 fwd conv_fwd_mfma<64,32,.,9> (2048 tiles)
    3 x 21847  M = 65541                            the same, other side         fwd conv_fwd_mfma<.,.,.,9>, 64 -> 64 <64,64,.,3> + combine ("big");
                                                                                 dx conv_dx_mfma<32,.,9>, 64 -> 32 / 64 -> 64 <64,.,3> + combine
                                                                                 ("big"); dW conv_dw_mfma + conv_dw_reduce; bwd "two"
    3 x 22001, rows 5500   M_dx = 66003             dx_is_lat: 2 dpre_rows <= m   dx conv_dx_lat above kLatMaxRows (32 -> 32 with CTW 2); bwd "lat"
                                                    (33000 <= 66003)             for cout 32
    3 x 22001, rows 13201                           the same (79206 > 66003)     dx conv_dx_mfma; bwd "two"
    3 x 911, rows 2733  (rows = 3 vsrc)             --                           dx conv_dx_ks with 27 entries per vertex on average, fwd conv_fwd_pt
    3 x 2731, rows 683  (Enblock form)              --                           dx conv_dx_lat with most keys empty; fwd conv_fwd_ks
    small shapes at 1 x 37, 3 x 2731, 3 x 21847     grid caps 65536 (3 -> 16 and  conv_fwd_in_mfma / conv_dw_in_mfma<1|2|3, 32|64>, conv_fwd_in_small /
              and 3 x 44001 (3 -> 32, 32 -> 3)      64 -> 3 dW), 131072 (3 -> 32, conv_dw_in_small<3,16>, conv_fwd_out_small / conv_dx_out_small /
                                                    32 -> 3 dW, small_grid)      conv_dw_out_small<16|32|64, 3>, slab_reduce
    small 3 -> 32, 16 -> 3 at 3 x 87401 M = 262203   grid caps at 262144 rows     conv_fwd_in_mfma (2048 workgroups), conv_dw_out_small<16,3> (512)
    fused 32/64 -> 1/2/3 at 1 x 37, 3 x 2731,       --                           conv_bwd_out_mfma<32|64, 1|2|3> with and without dx
              3 x 911 rows 2733, 3 x 2731 rows 683
    fused at 3 x 87401                              fused_small_gx: 262144 rows  the same on its capped grid of 1024 workgroups
    fused up 1 x 37, 3 x 2729; 3 x 2731 refused     kMaxTilesFew * 16            conv_fwd_pt<32,32,1>, <64,64,1>
    row subset, 32 -> 32 and 32 -> 64:
      3 x 149 rows 37, widths 4 8 12 16             rowsub_groups -> 18          conv_bwd_rowsub_pair + conv_dx_rowsub_gather<32, 1|2|3|4>
      3 x 3644 rows 911                             rowsub_groups: 171 tiles -> 9 the same, 9 column groups
      16 x 149 rows 37, 16 x 3644 rows 911          batch % 16 == 0              32 -> 32 widths 8 12 16: vm32::conv_bwd_flat_pair<32,32,8|12|16>
              (911 tiles -> 2 column groups)                                     and (data only) conv_dx_flat_vm32<32,32,8|12|16>; width 4 and
                                                                                 32 -> 64: dG + gather
      3 x 87388 rows 21847, width 8                 kLatDwMax = 65536            conv_bwd_rowsub_pair (1 column group: 78 KB of W^T in LDS at
                                                                                 32 -> 64) dG only, conv_dw_mfma, gather

Tables: every line above runs with ``hubs`` and with ``head_edge`` (which has the ``gaps``) except
1 x 37 (``head_edge``: ``hubs`` needs 160 vertices), the rows != vsrc lines (``one_vertex_rows`` and
``random`` as well) and the row-subset lines, whose flat lists cannot be hubs (fan-in <= 16):
``fan_table`` with its own gaps.

Not covered, with the reason:
  * conv_fwd_mfma<.,.,.,1> and conv_dx_mfma<.,.,1>, conv_dx_mfma<32,.,3>, conv_fwd_mfma<32,.,.,3>: pick_spg
    gives 1 slot per group below 400 tiles and 3 below 2048, but every such forward is taken by the coarse
    kernels (M < 24576) or conv_fwd_lat (M < 65536, 64 -> 32 excepted), every such dx by conv_dx_ks /
    conv_dx_lat: unreachable from the entry points.
  * conv_bwd_lat_pair<64,32,1> (LatPairShapes x LatPairCtws): dx_lat_ctw(64, 32) is the constant 2.
  * conv_dw_in_small<3,32>, <3,64> (InSmallShapes): dw_geom gives cin <= 3, cout 32 / 64 to conv_dw_in_mfma.
  * conv_fwd_out_small<32,1>, <32,2> (OutSmallShapes): taken by cfsd_spiral_conv_fwd_x alone (out of scope).
  * the bf16 and vertex-major entry points: ``test_gpu_vertex_major_conv`` and ``test_gpu_bf16_conv`` (exact-value
    inputs and a rounding model of their own).
"""
import ctypes

import numpy as np
import pytest
import torch

import spiral_tables as T
from conv_cases import ACT_ELU, ACT_NONE, DEV, U, Case, check, gamma
from craniofacialsd_vae_amd import _abi, ops, topology

pytestmark = pytest.mark.gpu

SEQ = 9
KS_MAX = 512 * 16      # coarse::kMaxTilesFew * 16: slot-group dx / fused up below
MFMA = [(32, 32), (32, 64), (64, 32), (64, 64)]
NAN = float("nan")
CHUNK = 4096           # rows per step of the fp64 restatement (a [3, 4096, 576] fp64 operand: 57 MB)


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def nan_ws(nbytes):
    return nan(nbytes // 4 + 1)


def chk(name, got, ref, tol, shape):
    assert bool(torch.isfinite(got).all()), (name, shape, "non-finite element (left unwritten?)")
    return check(name, got, ref, tol, shape)


TABLES = {"random": T.random, "hubs": T.hubs, "head_edge": T.head_edge, "one_vertex_rows": T.one_vertex_rows}


def make_case(batch, vsrc, rows, cin, cout, table):
    idx = TABLES[table](rows, vsrc, seed=cin + cout)
    seed = (batch * 7 + vsrc) * 131 + rows * 17 + cin * 3 + cout
    c = Case(batch, vsrc, rows, SEQ, cin, cout, seed=seed, idx=idx, chunk=CHUNK, elu_edges=True)
    if table == "head_edge":
        assert bool(c.absent_all[0]) and bool(c.absent_all[vsrc - 1])
    c.g0 = (c.elu_y == -1.0).to(DEV)
    assert bool(c.g0.any()) and bool((c.elu_y == 0.0).any())
    return c


def n_dx_inverse(c):
    """The inverse-table dx kernels' rounding count per source vertex (module docstring)."""
    _, vsrc, _, _, _, cout = c.shape
    cnt = torch.from_numpy(T.key_counts(c.idx.numpy(), vsrc))
    n = cnt.max(1).values - 1 + cout * (cnt > 0).sum(1)
    n[cnt.sum(1) == 0] = 0
    assert bool((n.double().view(1, vsrc, 1) <= c.n_dx).all())
    return n.double().view(1, vsrc, 1)


def tol_dx(c):
    return gamma(n_dx_inverse(c)) * c.dx_abs


def tol_dx_elu(c):
    tol = tol_dx(c)
    return c.g * tol + U * (c.ref_dx_elu().abs() + c.g * tol)


def has(role, c):
    return ops.spiral_conv_has_shape(role, SEQ, c.shape[4], c.shape[5])


def assert_exact_zeros(c, dx, with_elu):
    """dx of a vertex in no spiral, and under ELU' = 0, is exactly 0."""
    absent = c.absent_all.to(DEV)
    assert torch.count_nonzero(dx[:, absent]) == 0
    if with_elu:
        assert torch.count_nonzero(dx[c.g0]) == 0


# ------------------------------------------------------------------ the separate entry points
def run_separate(c):
    batch, vsrc, rows, seq, cin, cout = c.shape
    d, out = c.d, {}
    need = ops.spiral_conv_workspace(batch, vsrc, rows, seq, cin, cout)
    if has(ops.CONV_FWD, c):
        for key, act in (("y_none", ACT_NONE), ("y_elu", ACT_ELU)):
            out[key] = ops.spiral_conv_fwd(d["x"], d["idx"], d["w"], d["b"], act, out=nan(batch, rows, cout),
                                           workspace=nan_ws(need))
    if has(ops.CONV_BWD_DATA, c):
        out["dx"] = ops.spiral_conv_bwd_data(d["dpre"], c.inv, d["w"], vsrc, out=nan(batch, vsrc, cin),
                                             workspace=nan_ws(need))
        out["dx_elu"] = ops.spiral_conv_bwd_data(d["dpre"], c.inv, d["w"], vsrc, elu_y=d["elu_y"],
                                                 out=nan(batch, vsrc, cin), workspace=nan_ws(need))
    if has(ops.CONV_BWD_WEIGHT, c):
        need_w = ops.spiral_conv_bwd_weight_workspace(batch, rows, seq, cin, cout)
        assert need_w > 0
        out["dw"], out["db"] = nan(cout, seq * cin), nan(cout)
        assert ops.spiral_conv_bwd_weight(d["x"], d["idx"], d["dpre"], out["dw"], out["db"], nan_ws(need_w)) is None
        item = ops.spiral_conv_bwd_weight(d["x"], d["idx"], d["dpre"], None, None, nan_ws(need_w))
        assert isinstance(item, ops.DeferredDw)
        out["dw_deferred"], out["db_deferred"] = nan(cout, seq * cin), nan(cout)
        ops.dw_reduce_batch([(item, out["dw_deferred"], out["db_deferred"])])
    return out


def check_separate(c, out):
    s = c.shape
    if "y_none" in out:
        chk("fwd", out["y_none"], c.pre, c.tol_fwd(), s)
        chk("fwd+elu", out["y_elu"], c.ref_elu(), c.tol_fwd_elu(), s)
    if "dx" in out:
        chk("dx", out["dx"], c.dx, tol_dx(c), s)
        chk("dx*elu'", out["dx_elu"], c.ref_dx_elu(), tol_dx_elu(c), s)
        assert_exact_zeros(c, out["dx"], False)
        assert_exact_zeros(c, out["dx_elu"], True)
    if "dw" in out:
        chk("dw", out["dw"], c.dw, c.tol_dw(), s)
        chk("db", out["db"], c.db, c.tol_db(), s)
        assert torch.equal(out["dw_deferred"], out["dw"]) and torch.equal(out["db_deferred"], out["db"])


def separate_case(c):
    out = run_separate(c)
    assert out, c.shape
    check_separate(c, out)
    again = run_separate(c)
    for k in out:
        assert torch.equal(out[k], again[k]), (k, c.shape)


# ------------------------------------------------------------------ cfsd_spiral_conv_bwd
def run_bwd(c, with_dx, elu, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    d = c.d
    ws = nan_ws(ops.spiral_conv_bwd_workspace(batch, vsrc, rows, seq, cin, cout))
    dx = nan(batch, vsrc, cin) if with_dx else None
    dw, db = nan(cout, seq * cin), nan(cout)
    ey = d["elu_y"] if elu else None
    if not deferred:
        r = ops.spiral_conv_bwd(d["x"], d["idx"], d["dpre"], c.inv, d["w"], dw, db, dx=dx, elu_y=ey, workspace=ws)
        assert r is dx
    else:
        r = ops.spiral_conv_bwd(d["x"], d["idx"], d["dpre"], c.inv, d["w"], None, None, dx=dx, elu_y=ey, workspace=ws)
        assert r[0] is dx and isinstance(r[1], ops.DeferredDw)
        ops.dw_reduce_batch([(r[1], dw, db)])
    return dx, dw, db


def bwd_case(c):
    """``ops.spiral_conv_bwd`` with dx (with and without ELU') and without, immediate and deferred."""
    s = c.shape
    for with_dx, elu in ((True, False), (True, True), (False, False)):
        dx, dw, db = run_bwd(c, with_dx, elu, False)
        tag = "fused" + (" (no dx)" if not with_dx else "")
        chk(tag + " dw", dw, c.dw, c.tol_dw(), s)
        chk(tag + " db", db, c.db, c.tol_db(), s)
        if with_dx:
            if elu:
                chk("fused dx*elu'", dx, c.ref_dx_elu(), tol_dx_elu(c), s)
            else:
                chk("fused dx", dx, c.dx, tol_dx(c), s)
            assert_exact_zeros(c, dx, elu)
        dx2, dw2, db2 = run_bwd(c, with_dx, elu, True)   # deferred == immediate, bit for bit
        assert torch.equal(dw2, dw) and torch.equal(db2, db)
        dx3, dw3, db3 = run_bwd(c, with_dx, elu, False)  # a second call: bit-identical
        assert torch.equal(dw3, dw) and torch.equal(db3, db)
        if with_dx:
            assert torch.equal(dx2, dx) and torch.equal(dx3, dx)


def pair_kind(c):
    batch, vsrc, rows, seq, cin, cout = c.shape
    if not ops.spiral_conv_bwd_paired(batch, vsrc, rows, seq, cin, cout):
        return "two"
    return "ks" if batch * vsrc < KS_MAX else "lat"


# (batch, vsrc, rows, tables, shapes, {shape: expected pair kind})
def _kinds(cout32, cout64):
    return {(32, 32): cout32, (64, 32): cout32, (32, 64): cout64, (64, 64): cout64}


BOTH = ("hubs", "head_edge")
MFMA_CASES = [
    (1, 37, 37, ("head_edge",), MFMA, _kinds("ks", "ks")),
    (3, 2729, 2729, BOTH, MFMA, _kinds("ks", "ks")),
    (3, 2731, 2731, BOTH, MFMA, _kinds("lat", "two")),
    (3, 8191, 8191, BOTH, MFMA, _kinds("lat", "two")),
    (3, 8193, 8193, BOTH, MFMA, _kinds("lat", "two")),
    (3, 10923, 10923, BOTH, [(32, 32)], _kinds("lat", "two")),
    (3, 21845, 21845, BOTH, MFMA, _kinds("lat", "two")),
    (3, 21847, 21847, BOTH, MFMA, _kinds("two", "two")),
    (3, 22001, 5500, BOTH, MFMA, _kinds("lat", "two")),
    (3, 22001, 13201, BOTH, MFMA, _kinds("two", "two")),
    (3, 911, 2733, BOTH + ("one_vertex_rows",), MFMA, _kinds("ks", "ks")),
    (3, 2731, 683, BOTH + ("random",), MFMA, _kinds("lat", "two")),
]
MFMA_PARAMS = [pytest.param(b, v, r, t, ci, co, kinds[(ci, co)], id=f"{b}x{v}-rows{r}-{ci}to{co}-{t}")
               for b, v, r, tables, shapes, kinds in MFMA_CASES for t in tables for ci, co in shapes]


@pytest.mark.parametrize("batch,vsrc,rows,table,cin,cout,kind", MFMA_PARAMS)
def test_mfma_shapes(batch, vsrc, rows, table, cin, cout, kind):
    """Forward, dx, dW through the separate entry points and through ``ops.spiral_conv_bwd``; the
    pairing query says which backward launch the case takes (slot-group pair, latency pair, two)."""
    c = make_case(batch, vsrc, rows, cin, cout, table)
    assert all(has(r, c) for r in (ops.CONV_FWD, ops.CONV_BWD_DATA, ops.CONV_BWD_WEIGHT))
    assert pair_kind(c) == kind
    separate_case(c)
    bwd_case(c)


def test_forward_64_32_with_a_short_workspace():
    """64 -> 32 at 24 579 rows is the slot-group forward: 3 slots per group with the workspace of
    the query; with one float less than 3 groups need, pick_spg's loop falls back to 9 slots in one
    group (no combine).  Both within the forward bound."""
    c = make_case(3, 8193, 8193, 64, 32, "hubs")
    batch, vsrc, rows, seq, cin, cout = c.shape
    d = c.d
    need = ops.spiral_conv_workspace(batch, vsrc, rows, seq, cin, cout)
    three_groups = 3 * batch * rows * cout * 4
    assert three_groups <= need
    for nbytes in (need, three_groups - 4):
        ws = nan(nbytes // 4)
        y = nan(batch, rows, cout)
        ops.call("cfsd_spiral_conv_fwd", ops.ptr(d["x"]), ops.ptr(d["idx"]), ops.ptr(d["w"]), ops.ptr(d["b"]),
                 ops.ptr(y), ops.ptr(ws), ctypes.c_size_t(ws.numel() * 4), batch, vsrc, rows, seq, cin, cout, ACT_ELU,
                 ops.stream_ptr())
        chk(f"fwd+elu (workspace {nbytes} B)", y, c.ref_elu(), c.tol_fwd_elu(), c.shape)


# ------------------------------------------------------------------ small-channel shapes
IN_SHAPES = [(1, 32), (2, 32), (3, 32), (1, 64), (2, 64), (3, 64), (3, 16)]   # forward and dW
OUT_SHAPES = [(16, 3), (32, 3), (64, 3)]                    # forward, dx and dW
SMALL_CASES = [
    (1, 37, 37, ("head_edge",), IN_SHAPES + OUT_SHAPES),
    (3, 2731, 2731, BOTH, IN_SHAPES + OUT_SHAPES),
    (3, 21847, 21847, BOTH, IN_SHAPES + OUT_SHAPES),
    (3, 44001, 44001, BOTH, [(3, 32), (32, 3)]),
    (3, 87401, 87401, BOTH, [(3, 32), (16, 3)]),
    (3, 911, 2733, ("one_vertex_rows",), OUT_SHAPES),
    (3, 2731, 683, ("random",), OUT_SHAPES),
]
SMALL_PARAMS = [pytest.param(b, v, r, t, ci, co, id=f"{b}x{v}-rows{r}-{ci}to{co}-{t}")
                for b, v, r, tables, shapes in SMALL_CASES for t in tables for ci, co in shapes]


@pytest.mark.parametrize("batch,vsrc,rows,table,cin,cout", SMALL_PARAMS)
def test_small_channel_shapes(batch, vsrc, rows, table, cin, cout):
    c = make_case(batch, vsrc, rows, cin, cout, table)
    assert has(ops.CONV_FWD, c) and has(ops.CONV_BWD_WEIGHT, c)
    assert has(ops.CONV_BWD_DATA, c) == (cout == 3)
    separate_case(c)


FUSED_SHAPES = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3)]
FUSED_CASES = [
    (1, 37, 37, ("head_edge",)),
    (3, 2731, 2731, BOTH),
    (3, 911, 2733, ("one_vertex_rows", "hubs")),
    (3, 2731, 683, ("head_edge", "random")),
    (3, 87401, 87401, ("hubs",)),
]
FUSED_PARAMS = [pytest.param(b, v, r, t, ci, co, id=f"{b}x{v}-rows{r}-{ci}to{co}-{t}")
                for b, v, r, tables in FUSED_CASES for t in tables for ci, co in FUSED_SHAPES]


@pytest.mark.parametrize("batch,vsrc,rows,table,cin,cout", FUSED_PARAMS)
def test_fused_small_output_backward(batch, vsrc, rows, table, cin, cout):
    c = make_case(batch, vsrc, rows, cin, cout, table)
    assert has(ops.CONV_BWD_FUSED, c) and pair_kind(c) == "two"
    bwd_case(c)


# ------------------------------------------------------------------ fused up-sampling forward
def up_matrix(rows, n_coarse, seed):
    """An up-sampling matrix of 1 to 3 entries per row as [rows, 3] columns / values (a missing
    entry: column 0, value 0)."""
    rs = np.random.RandomState(seed)
    col = rs.randint(0, n_coarse, size=(rows, 3))
    val = rs.uniform(0.1, 1.0, size=(rows, 3)).astype(np.float32)
    n = rs.randint(1, 4, size=rows)
    n[:3] = [1, 2, 3]
    gone = np.arange(3)[None, :] >= n[:, None]
    col[gone], val[gone] = 0, 0.0
    return col, val


@pytest.mark.parametrize("table", ["hubs", "head_edge"])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64)])
@pytest.mark.parametrize("batch,rows", [(1, 37), (3, 2729)])
def test_fused_up_forward(batch, rows, cin, cout, table):
    """``ops.spiral_conv_fwd_up`` against Pool(up) then the conv in fp64, and the up-sampled rows it
    stores (slot 0 of a spiral is the vertex itself, as ``DeviceTopology.up_comp`` requires)."""
    if rows < 160:
        table = "head_edge"
    assert ops.spiral_conv_fwd_up_supported(batch, rows, SEQ, cin, cout) and batch * rows < KS_MAX
    n_coarse = (rows + 3) // 4
    idx = TABLES[table](rows, rows, seed=cin)
    idx[:, 0] = np.arange(rows)
    col, val = up_matrix(rows, n_coarse, seed=rows + cin)
    g = torch.Generator().manual_seed(rows + cout)
    xc = torch.randn(batch, n_coarse, cin, generator=g)
    w = torch.randn(cout, SEQ * cin, generator=g)
    b = torch.randn(cout, generator=g)
    colt, valt = torch.from_numpy(col), torch.from_numpy(val).double()
    up = sum(valt[:, k].view(1, rows, 1) * xc.double()[:, colt[:, k]] for k in range(3))
    up_abs = sum(valt[:, k].view(1, rows, 1) * xc.double().abs()[:, colt[:, k]] for k in range(3))
    flat = torch.from_numpy(idx).reshape(-1)
    pre = up[:, flat].reshape(batch, rows, -1) @ w.double().T + b.double()
    pre_abs = up_abs[:, flat].reshape(batch, rows, -1) @ w.double().abs().T + b.double().abs()
    tol = gamma(SEQ * cin + 1 + 3) * pre_abs
    comp = (torch.from_numpy(np.ascontiguousarray(col[idx], np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(val[idx], np.float32)).to(DEV))
    shape = (batch, n_coarse, rows, SEQ, cin, cout)
    dv = [t.to(DEV) for t in (xc, torch.from_numpy(idx).to(torch.int32), w, b)]
    outs = []
    for rep in range(2):
        for act in (ACT_NONE, ACT_ELU):
            y, yup = nan(batch, rows, cout), nan(batch, rows, cin)
            ops.spiral_conv_fwd_up(dv[0], comp, dv[1], dv[2], dv[3], act, out=y, up_out=yup)
            outs.append((y, yup))
            if rep:
                continue
            chk("up rows", yup, up, gamma(3) * up_abs, shape)
            if act == ACT_NONE:
                chk("up fwd", y, pre, tol, shape)
            else:
                ref = torch.where(pre > 0, pre, torch.expm1(pre))
                chk("up fwd+elu", y, ref, tol + U * ref.abs().clamp_min(1.0), shape)
    for (y, yup), (y2, yup2) in zip(outs[:2], outs[2:]):
        assert torch.equal(y, y2) and torch.equal(yup, yup2)
    y = nan(batch, rows, cout)                       # without up_out
    ops.spiral_conv_fwd_up(dv[0], comp, dv[1], dv[2], dv[3], ACT_ELU, out=y)
    assert torch.equal(y, outs[1][0])


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64)])
def test_fused_up_refused_above_the_few_tile_limit(cin, cout):
    batch, rows = 3, 2731
    assert batch * rows >= KS_MAX and not ops.spiral_conv_fwd_up_supported(batch, rows, SEQ, cin, cout)
    n_coarse = 683
    z = torch.zeros
    comp = (z(rows, SEQ, 3, dtype=torch.int32, device=DEV), z(rows, SEQ, 3, device=DEV))
    y = nan(batch, rows, cout)
    with pytest.raises(_abi.CfsdError):
        ops.spiral_conv_fwd_up(z(batch, n_coarse, cin, device=DEV), comp, z(rows, SEQ, dtype=torch.int32, device=DEV),
                               z(cout, SEQ * cin, device=DEV), z(cout, device=DEV), ACT_ELU, out=y)
    assert bool(torch.isnan(y).all())  # refused before any launch


# ------------------------------------------------------------------ row-subset backward
def make_rowsub_case(batch, vsrc, rows, cout, fan):
    idx = T.fan_table(rows, vsrc, fan, seed=fan + cout)
    c = Case(batch, vsrc, rows, SEQ, 32, cout, seed=vsrc + 13 * rows + fan + cout + batch, idx=idx, chunk=CHUNK,
             elu_edges=True)
    c.g0 = (c.elu_y == -1.0).to(DEV)
    table, width = topology.inverse_flat(idx, vsrc)
    assert width == fan and bool(c.absent_all[0]) and bool(c.absent_all[vsrc - 1])
    c.flat = (torch.from_numpy(table).to(DEV), width)
    return c


def run_rowsub(c, elu, deferred):
    batch, vsrc, rows, seq, cin, cout = c.shape
    d = c.d
    ws = nan_ws(ops.spiral_conv_bwd_rowsub_workspace(batch, vsrc, rows, seq, cin, cout))
    dx, dw, db = nan(batch, vsrc, cin), nan(cout, seq * cin), nan(cout)
    ey = d["elu_y"] if elu else None
    if not deferred:
        r = ops.spiral_conv_bwd_rowsub(d["x"], d["idx"], d["dpre"], c.flat, d["w"], dw, db, dx, elu_y=ey, workspace=ws)
        assert r is dx
    else:
        r = ops.spiral_conv_bwd_rowsub(d["x"], d["idx"], d["dpre"], c.flat, d["w"], None, None, dx, elu_y=ey,
                                       workspace=ws)
        assert r[0] is dx and isinstance(r[1], ops.DeferredDw)
        ops.dw_reduce_batch([(r[1], dw, db)])
    return dx, dw, db


def run_rowsub_data(c, elu):
    batch, vsrc, rows, seq, cin, cout = c.shape
    ws = nan_ws(ops.spiral_conv_bwd_data_rowsub_workspace(batch, rows, seq, cin))
    return ops.spiral_conv_bwd_data_rowsub(c.d["dpre"], c.flat, c.d["w"], vsrc, elu_y=c.d["elu_y"] if elu else None,
                                           out=nan(batch, vsrc, cin), workspace=ws)


ROWSUB_GEOMS = [(3, 149, 37), (3, 3644, 911), (16, 149, 37), (16, 3644, 911)]


@pytest.mark.parametrize("fan", [4, 8, 12, 16])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("batch,vsrc,rows", ROWSUB_GEOMS)
def test_row_subset_backward(batch, vsrc, rows, cout, fan):
    """``ops.spiral_conv_bwd_rowsub`` and ``ops.spiral_conv_bwd_data_rowsub`` at every flat-list
    width.  Batch 3: dG + gather.  Batch 16, 32 -> 32, widths 8 / 12 / 16: the flat-list MFMA kernels
    (their dx equals the dG path's to fp32 rounding only: the bound, not ``torch.equal``)."""
    c = make_rowsub_case(batch, vsrc, rows, cout, fan)
    rowsub_case(c)


@pytest.mark.parametrize("cout,fan", [(32, 8), (64, 12)])
def test_row_subset_backward_many_rows(cout, fan):
    """65 541 rows: the dW half is the persistent conv_dw_mfma behind a dG-only launch, and the dG
    tiles take one column group (rowsub_groups: 4097 row tiles >= 1536)."""
    rowsub_case(make_rowsub_case(3, 87388, 21847, cout, fan))


def rowsub_case(c):
    s = c.shape
    assert ops.spiral_conv_bwd_rowsub_workspace(*s) > 0
    for elu in (False, True):
        ref, tol = (c.ref_dx_elu(), c.tol_dx_elu()) if elu else (c.dx, c.tol_dx())
        tag = "*elu'" if elu else ""
        dx, dw, db = run_rowsub(c, elu, False)
        chk("rowsub dx" + tag, dx, ref, tol, s)
        chk("rowsub dw", dw, c.dw, c.tol_dw(), s)
        chk("rowsub db", db, c.db, c.tol_db(), s)
        assert_exact_zeros(c, dx, elu)
        dx2, dw2, db2 = run_rowsub(c, elu, True)    # deferred == immediate, bit for bit
        assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)
        dx3, dw3, db3 = run_rowsub(c, elu, False)   # a second call: bit-identical
        assert torch.equal(dx3, dx) and torch.equal(dw3, dw) and torch.equal(db3, db)
        dxd = run_rowsub_data(c, elu)
        chk("rowsub data-only dx" + tag, dxd, ref, tol, s)
        assert_exact_zeros(c, dxd, elu)
        assert torch.equal(run_rowsub_data(c, elu), dxd)
