"""Which launches each conv layer's backward takes, decided once per batch size.

``build`` gives the output conv, each Deblock conv and each Enblock conv one
:class:`Layer` record holding the first KIND of its family that applies.  A
kind is one function below (the layer's launches; returns its deferred
weight-gradient slab set); ``@kind`` registers it with its ``applies`` test
and its ``workspace`` query.  ``SDVAEEngine.buffers`` sizes ``b.ws_dw`` from
the plan and backward_head / backward_tail run it: sizing and dispatch cannot
disagree.  The figures are the measurements (MI355X, batch 16) that put a
fused launch in front of the separate ones it replaces.
"""
import torch

from . import ops


class Layer:
    """One conv layer's backward: ``key`` (of ``b.plan`` / ``b.ws_dw``), parameter ``name``,
    level, shape, spiral table ``idx``, inverse CSR ``inv``, flat inverse list ``flat`` (or
    None), ``operands`` (x, dpre, dx, elu_y), the chosen ``kind``, ``nbytes`` of its region."""

    def __init__(self, eng, b, key, name, cin, cout, lv, idx, inv, flat, rows, operands, kinds):
        T = eng.topo
        self.key, self.name, self.cin, self.cout, self.lv, self.operands = key, name, cin, cout, lv, operands
        self.idx, self.inv, self.flat = idx, inv, flat
        self.bsz, self.vsrc, self.rows, self.seq = b.bsz, T.n_verts[lv], rows, T.seq[lv]
        self.shape = (b.bsz, self.vsrc, rows, self.seq, cin, cout)
        self.vm = lv in b.xl                         # operands vertex-major ...
        self.bf16 = self.vm and bool(eng.lp_levels)  # ... and bf16
        # a batch-major layer whose backward the specialised entry points refuse (another spiral
        # length or channel pair): the general-shape kernels.  They are fp32 batch-major only, so
        # never a vertex-major layer (vm_levels and the bf16 check admit only shapes with instances)
        self.general = not self.vm and ops.spiral_conv_bwd_is_general(self.seq, cin, cout, dx=operands[2] is not None)
        enc = key[0] == "enc"
        # Enblock whose input is the previous Enblock's ELU output (else Pool(down)^T follows)
        self.sel_prev = enc and lv > 0 and T.enc_select[lv - 1]
        self.flat_dx = key[0] == "dec" and eng._flat_dx(b, lv, cin, cout)
        # vertex-major Enblock whose dpre is fp32 batch-major: dx as dG = dpre.W at the
        # kept rows (fp32, in b.ws) + the flat gather, rounded once to the level's dtype
        self.dg_bytes = 0
        if enc and self.vm and lv > 0 and flat is not None and lv + 1 not in b.xl:
            self.dg_bytes = ops.spiral_conv_bwd_data_rowsub_workspace(b.bsz, rows, self.seq, cin)
        self.kind, self.workspace = next((k, query) for k, applies, query in kinds if applies(self, eng))
        self.nbytes = self.workspace(self)

    def run(self, eng, b, items):
        """Issue the kind's launches; the deferred weight-gradient slab set joins ``items``."""
        P, w = eng.params, self.name + ".weight"
        d = self.kind(self, b.ws_dw[self.key], P.view(w), eng._wx(w), b.ws, *self.operands)
        items.append((d, P.gview(w), P.gview(self.name + ".bias")))


OUT_KINDS, DEC_KINDS, ENC_KINDS = [], [], []  # (kind, applies, workspace query), in the order they are tried


def kind(families, applies, workspace):
    def register(fn):
        for f in families:
            f.append((fn, applies, workspace))
        return fn
    return register


def _weight_x_bytes(L):
    xdt = torch.bfloat16 if L.bf16 and L.cin > 3 else torch.float32
    return ops.spiral_conv_bwd_weight_x_workspace(L.bsz, L.rows, L.seq, L.cin, L.cout, xdt)


_pair_bytes = lambda L: ops.spiral_conv_bwd_flat_pair_workspace(L.bsz, L.rows, L.seq, L.cin, L.cout)  # noqa: E731
_flat_pair_bytes = lambda L: max(_weight_x_bytes(L), _pair_bytes(L))  # noqa: E731
_bwd_bytes = lambda L: ops.spiral_conv_bwd_workspace(*L.shape)  # noqa: E731
_rowsub_bytes = lambda L: ops.spiral_conv_bwd_rowsub_workspace(*L.shape)  # noqa: E731


_weight_bytes = lambda L: ops.spiral_conv_bwd_weight_workspace(L.bsz, L.rows, L.seq, L.cin, L.cout)  # noqa: E731


# kind(L, region, w, wx, ws, x, dpre, dx, elu_y): region = b.ws_dw[key]; w the fp32 weight, wx the
# weight the vertex-major kernels read (bf16 shadow in bf16 mode); ws = b.ws
@kind([OUT_KINDS, DEC_KINDS, ENC_KINDS], lambda L, e: L.general, _weight_bytes)
def general(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """A shape without a specialised instance (spiral length other than 9, channels outside the
    lists): dW slabs, then dx, each on the general-shape kernels where the product has no instance
    (ops routes per product).  Tried first; applies only to a batch-major layer whose backward the
    specialised entry points refuse, so the plan of every layer they take is unchanged."""
    d = ops.spiral_conv_bwd_weight(x, L.idx, dpre, None, None, region)
    if dx is not None:
        ops.spiral_conv_bwd_data(dpre, L.inv, w, L.vsrc, elu_y=elu_y, out=dx, workspace=ws)
    return d


@kind([OUT_KINDS], lambda L, e: L.vm and L.bsz % 16 == 0 and L.cin == 32 and L.cout == 3 and L.flat is not None,
      _bwd_bytes)
def out_flat(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Output conv 32 -> 3, vertex-major level 0, batch % 16: dx + dW along each vertex's flat inverse list."""
    return ops.spiral_conv_bwd_out_flat(x, L.idx, dpre, L.flat, w, None, None, dx=dx, elu_y=elu_y,
                                        workspace=region)[1]


@kind([OUT_KINDS], lambda L, e: L.vm, _bwd_bytes)
def out_x(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Output conv with vertex-major (fp32 or bf16) operands: dx + dW through the inverse CSR."""
    return ops.spiral_conv_bwd_x(x, L.idx, dpre, L.inv, w, None, None, dx=dx, elu_y=elu_y, workspace=region)[1]


@kind([DEC_KINDS], lambda L, e: L.bf16 and L.cout == 32 and L.flat_dx and L.lv in e.vm_pair_levels16,
      _flat_pair_bytes)
def flat_pair16(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """bf16 Deblock 32 -> 32: flat dx + dW slabs in one launch, at both vertex-major levels
    (D3 29.0 vs 20.0 + 19.0 us, D2 14.7 vs 10.4 + 11.6 us, step 0.427 -> 0.409 ms)."""
    return ops.spiral_conv_bwd_flat_pair_bf16(x, L.idx, dpre, L.flat, wx, dx, workspace=region)


@kind([DEC_KINDS], lambda L, e: (L.vm and not L.bf16 and L.cout == 32 and L.flat_dx and L.lv in e.vm_pair_levels
                                 and _pair_bytes(L) > 0), _flat_pair_bytes)
def flat_pair32(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """fp32 vertex-major Deblock 32 -> 32: the same pair, at level 1 only (D2: 37.8 vs 20.8 +
    19.9 us, step 0.563 vs 0.568 ms same-box); at level 0 the pair is slower (117.5 vs 51.4 +
    52.0 us: the dx role's 12-wave workgroups lose to its 2-per-CU kernel)."""
    return ops.spiral_conv_bwd_flat_pair(x, L.idx, dpre, L.flat, w, None, None, dx, workspace=region)


@kind([DEC_KINDS], lambda L, e: L.flat_dx, _weight_x_bytes)
def weight_x_flat(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Vertex-major Deblock, batch % 16: dW slabs, then dx with one MFMA per flat-list entry."""
    d = ops.spiral_conv_bwd_weight_x(x, L.idx, dpre, None, None, region)
    ops.spiral_conv_bwd_data_flat(dpre, L.flat, wx, L.vsrc, out=dx)
    return d


@kind([ENC_KINDS], lambda L, e: (L.bf16 and e.rowsub_pair16 and L.dg_bytes > 0 and L.sel_prev and L.cin == 32
                                 and L.cout == 32 and L.bsz % 16 == 0 and L.flat[1] <= 16), _weight_x_bytes)
def rowsub_pair16(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """bf16 Enblock 32 -> 32 on a row subset: its dG + flat-gather dx and its dW slabs in one
    launch (part of the bf16 step's 0.427 -> 0.409 ms)."""
    return ops.spiral_conv_bwd_rowsub_pair_bf16(x, L.idx, dpre, L.flat, w, dx, elu_y=elu_y, workspace=region)


@kind([ENC_KINDS], lambda L, e: (L.operands[2] is not None and L.flat is not None and _rowsub_bytes(L) > 0 and
                                 (not L.vm or (not L.bf16 and L.sel_prev and L.bsz * L.rows < 65536))),
      _rowsub_bytes)
def rowsub(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Enblock conv on a row subset: dG at the kept rows + dW slabs in one launch, then the flat
    gather; x batch-major, or fp32 vertex-major (E1 of the fp32 step: few-row layers)."""
    return ops.spiral_conv_bwd_rowsub(x, L.idx, dpre, L.flat, w, None, None, dx=dx, elu_y=elu_y,
                                      workspace=region)[1]


@kind([ENC_KINDS], lambda L, e: L.vm and L.dg_bytes > 0, _weight_x_bytes)
def weight_x_rowsub(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Vertex-major Enblock with fp32 dpre: dW slabs, then the row-subset dG + flat gather."""
    d = ops.spiral_conv_bwd_weight_x(x, L.idx, dpre, None, None, region)
    ops.spiral_conv_bwd_data_rowsub(dpre, L.flat, w, L.vsrc, elu_y=elu_y, out=dx, workspace=ws)
    return d


@kind([DEC_KINDS, ENC_KINDS], lambda L, e: L.vm, _weight_x_bytes)
def weight_x_inv(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Any other vertex-major conv: dW slabs, then dx through the inverse CSR (none at encoder level 0)."""
    d = ops.spiral_conv_bwd_weight_x(x, L.idx, dpre, None, None, region)
    if dx is not None:
        ops.spiral_conv_bwd_data_x(dpre, L.inv, wx, L.vsrc, elu_y=elu_y, out=dx)
    return d


@kind([DEC_KINDS, ENC_KINDS], lambda L, e: L.operands[2] is not None and ops.spiral_conv_bwd_paired(*L.shape),
      _bwd_bytes)
@kind([OUT_KINDS], lambda L, e: True, _bwd_bytes)
def paired(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Batch-major conv the library pairs, and the fp32 batch-major output conv: dx + dW slabs in one launch."""
    return ops.spiral_conv_bwd(x, L.idx, dpre, L.inv, w, None, None, dx=dx, elu_y=elu_y, workspace=region)[1]


@kind([DEC_KINDS, ENC_KINDS], lambda L, e: True, _weight_bytes)
def plain(L, region, w, wx, ws, x, dpre, dx, elu_y):
    """Batch-major fallback: dW slabs, then dx (none at level 0 of the encoder)."""
    d = ops.spiral_conv_bwd_weight(x, L.idx, dpre, None, None, region)
    if dx is not None:
        ops.spiral_conv_bwd_data(dpre, L.inv, w, L.vsrc, elu_y=elu_y, out=dx, workspace=ws)
    return d


def build(eng, b):
    """{key: Layer} in weight-gradient region order: "out", ("dec", i), ("enc", level)."""
    T, S = eng.topo, eng.spec
    nv = T.n_verts
    # the output conv has no activation: dpre = dout; its dx goes through the last Deblock's ELU
    plan = {"out": Layer(eng, b, "out", f"de_layers.{S.n + 1}.layer", S.out_ch[0], S.in_ch, 0, T.spiral[0],
                         T.spiral_inv[0], T.spiral_flat[0], nv[0],
                         (b.dec_out[-1], b.dout, b.dpre_dec[-1], b.dec_out[-1]), OUT_KINDS)}
    for i, (cin, cout, lv, _) in enumerate(S.dec_layers()):
        plan["dec", i] = Layer(eng, b, ("dec", i), f"de_layers.{i + 1}.conv.layer", cin, cout, lv, T.spiral[lv],
                               T.spiral_inv[lv], T.spiral_flat[lv], nv[lv],
                               (b.dec_up[i], b.dpre_dec[i], b.g_dec_up[i], None), DEC_KINDS)
    for (cin, cout, lv) in S.enc_layers():
        sel, p = T.enc_select[lv], lv - 1
        # dx into the previous Enblock's ELU, or (no selection) into the input of Pool(down)^T
        dx = (None, None) if lv == 0 else (b.dpre_enc[p], b.enc_out[p]) if T.enc_select[p] else (b.g_pooled[p], None)
        plan["enc", lv] = Layer(eng, b, ("enc", lv), f"en_layers.{lv}.conv.layer", cin, cout, lv, T.enc_rows[lv],
                                T.enc_inv[lv], T.enc_flat[lv] if sel else None, nv[lv + 1] if sel else nv[lv],
                                (b.x if lv == 0 else b.enc_out[p], b.dpre_enc[lv], *dx), ENC_KINDS)
    return plan
