"""Case builder shared by the SpiralConv kernel tests (``test_gpu_general_conv``,
``test_gpu_specialised_conv``, ``test_gpu_vertex_major_conv``, ``test_gpu_bf16_conv``):
the inputs of one conv, its fp64 restatement (``exact_values.restate``:
index_select + matmul; dx by index_add_; dW by G^T.dY) and the per-element
bounds derived in ``test_gpu_general_conv``'s docstring, plus the layout / dtype
helpers of the vertex-major and bf16 entry points.  A plain module, no
fixtures: importing it loads libcfsd."""
import contextlib
import copy
import os

import numpy as np
import torch

import cfsd_loader
import exact_values
import spiral_tables

cfsd_loader.load()
from craniofacialsd_vae_amd import ops, topology  # noqa: E402
from craniofacialsd_vae_amd.ops import ACT_ELU, ACT_NONE  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
# Unit roundoff of bf16: 8 significand bits (7 stored), round to nearest even, so |fl(v) - v| <= 2^-8 |v| (the tie
# 1 + 2^-8 rounds to 1).  Half of that, 2^-9, holds only relative to the NEXT power of two: measured on the
# bf16 dx of conv_bwd_out_vm, whose rounding the exact-input cases prove bit for bit, max err / bound was 1.99
# under 2^-9 ("Testing the vertex-major and bf16 convs").
UB = 2.0 ** -8
BF = torch.bfloat16
NAN = float("nan")


def gamma(n, u=U):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * u / (1 - n * u)


class Case:
    """Inputs of one conv (host fp32 + device copies) and its fp64 restatement.

    ``idx``: a ready ``[rows, seq]`` index table (``spiral_tables``) instead of
    the draw with replacement; every vertex it leaves out is in ``absent_all``.
    ``chunk``: rows per step of the restatement (the gathered ``[batch, rows,
    seq * cin]`` fp64 operand then exists for ``chunk`` rows at a time); the
    sums are fp64 either way.  ``elu_edges``: some ``elu_y`` entries are set to
    exactly -1 (ELU' = 0) and exactly 0.  ``values``: "randn", or "exact" for the
    dyadic inputs of ``exact_values`` (``dpre_values``: the set dpre is drawn
    from) -- the caller asserts ``exact_values.assert_exact(c.ref)``.  ``bf16``:
    names among x, w, dpre, elu_y that are rounded to bf16 BEFORE the reference
    sees them (the host tensors stay fp32 and hold the rounded values).
    ``device``: None keeps everything on the host (no device copies: the CPU
    dry run of a case).  ``parts``: the products whose reference is computed
    ("fwd", "dx", "dw"; a test that runs one entry point asks for that one)."""

    def __init__(self, batch, vsrc, rows, seq, cin, cout, seed, idx=None, chunk=None, elu_edges=False,
                 values="randn", dpre_values=exact_values.DYADIC, bf16=(), device=DEV, parts=exact_values.ALL_PARTS):
        g = torch.Generator().manual_seed(seed)
        self.shape = (batch, vsrc, rows, seq, cin, cout)
        if idx is None:
            idx = torch.randint(0, vsrc, (rows, seq), generator=g)  # with replacement
            self.absent = vsrc - 1                                  # a vertex that is in no spiral
            idx[idx == self.absent] = 0
        else:
            idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
            assert idx.shape == (rows, seq) and int(idx.min()) >= 0 and int(idx.max()) < vsrc
            self.absent = None
        self.idx = idx
        self.absent_all = torch.bincount(idx.reshape(-1), minlength=vsrc) == 0
        assert values in ("randn", "exact")
        self.exact = values == "exact"
        if self.exact:
            for k, t in exact_values.exact_inputs(g, batch, vsrc, rows, seq, cin, cout, dpre_values).items():
                setattr(self, k, t)
        else:
            self.x = torch.randn(batch, vsrc, cin, generator=g)
            self.w = torch.randn(cout, seq * cin, generator=g)
            self.b = torch.randn(cout, generator=g)
            self.dpre = torch.randn(batch, rows, cout, generator=g)
            # ELU outputs as the forward kernels produce them: fl(fl(exp(v)) - 1) for v <= 0
            v = torch.randn(batch, vsrc, cin, generator=g)
            self.elu_y = torch.where(v > 0, v, torch.exp(v) - 1.0)
        for k in bf16:
            assert k in ("x", "w", "dpre", "elu_y")
            setattr(self, k, getattr(self, k).to(BF).float())
        if elu_edges:
            self.elu_y[:, 0::5, 0::3] = -1.0  # exp underflowed: g = 0
            self.elu_y[:, 1::5, 0::3] = 0.0   # v = 0: g = 1
        self._variants = {}
        if device is not None:
            inv = topology.inverse_spiral(idx.numpy(), vsrc)
            self.d = {k: getattr(self, k).to(device) for k in ("x", "w", "b", "dpre", "elu_y")}
            self.d["idx"] = idx.to(torch.int32).to(device)
            self.inv = tuple(torch.from_numpy(a).to(device) for a in inv)
        self._ref(chunk, parts)

    def dev(self, name, bf16=False, vm=False):
        """Device copy of operand ``name`` in the requested storage and layout (kept: the same
        tensor serves every call of the case)."""
        key = (name, bf16, vm)
        if key not in self._variants:
            self._variants[key] = put(getattr(self, name), bf16, vm)
        return self._variants[key]

    def on_device(self):
        """A shallow copy whose fp64 reference tensors live on the device, so that the bounds and
        comparisons of a large case run there (the host copies stay as they are)."""
        d = copy.copy(self)
        n_inv = self.n_dx_inverse()
        for k, v in vars(self).items():
            if torch.is_tensor(v) and v.dtype == torch.float64:
                setattr(d, k, v.to(DEV))
        d.n_dx_inverse = lambda: n_inv.to(DEV)
        return d

    def _ref(self, chunk=None, parts=exact_values.ALL_PARTS):
        batch, vsrc, rows, seq, cin, cout = self.shape
        self.ref = exact_values.restate(self.idx, self.x, self.w, self.b, self.dpre, chunk, parts)
        for k, t in self.ref.items():
            setattr(self, k, t)
        self.n_fwd = seq * cin + 1
        self.n_dx = (torch.bincount(self.idx.reshape(-1), minlength=vsrc) * cout).double().view(1, vsrc, 1)
        y = self.elu_y.double()
        self.g = torch.where(y > 0, torch.ones_like(y), y + 1)
        self.n_dw = batch * rows

    # the derived bounds (test_gpu_general_conv's docstring), one tensor per product
    def tol_fwd(self):
        return gamma(self.n_fwd) * self.pre_abs

    def ref_elu(self):
        return torch.where(self.pre > 0, self.pre, torch.expm1(self.pre))

    def tol_fwd_elu(self):
        return self.tol_fwd() + U * self.ref_elu().abs().clamp_min(1.0)

    def tol_dx(self):
        return gamma(self.n_dx) * self.dx_abs

    def ref_dx_elu(self):
        return self.g * self.dx

    def tol_dx_elu(self):
        tol = self.tol_dx()
        return self.g * tol + U * (self.ref_dx_elu().abs() + self.g * tol)

    def tol_dw(self):
        return gamma(self.n_dw) * self.dw_abs

    def tol_db(self):
        return gamma(self.n_dw) * self.db_abs

    # ---- the bf16 kernels (test_gpu_bf16_conv's docstring).  Their operands are bf16, so every
    # product is exact in fp32 and the chains above keep their counts; ``UM`` is the unit roundoff
    # assumed for one MFMA-accumulated step.
    def n_dx_inverse(self):
        """Rounding count of the inverse-table dx per source vertex (test_gpu_specialised_conv's
        docstring): max_s E_s - 1 list adds, then cout products for each of the S non-empty slots."""
        _, vsrc, _, seq, _, cout = self.shape
        keys = (self.idx * seq + torch.arange(seq)).reshape(-1)
        cnt = torch.bincount(keys, minlength=vsrc * seq).reshape(vsrc, seq)
        n = cnt.max(1).values - 1 + cout * (cnt > 0).sum(1)
        n[cnt.sum(1) == 0] = 0
        return n.double().view(1, vsrc, 1)

    def tol_dx_inverse_b16(self, dx_abs=None):
        """Inverse-table bf16 dx before its output rounding: the list sum in fp32, ONE rounding of
        A_s[u, o] to bf16 (UB * |A_s| |w| <= UB * dx_abs in all), then the MFMA chain."""
        dx_abs = self.dx_abs if dx_abs is None else dx_abs
        gm = gamma(self.n_dx_inverse(), UM)
        return (gm + UB * (1 + gm)) * dx_abs

    def tol_dx_flat_b16(self):
        return gamma(self.n_dx, UM) * self.dx_abs

    def tol_fwd_b16(self):
        return gamma(self.n_fwd, UM) * self.pre_abs

    def tol_dw_b16(self):
        return gamma(self.n_dw, UM) * self.dw_abs

    def tol_db_b16(self):
        return gamma(self.n_dw, UM) * self.db_abs

    def with_elu_grad(self, ref, tol):
        """(g * ref, bound) after the multiplication by ELU' (one more fp32 rounding)."""
        return self.g * ref, self.g * tol + U * ((self.g * ref).abs() + self.g * tol)


UM = 2.0 ** -24  # MFMA-accumulated chains: see DESIGN.md "Testing the vertex-major and bf16 convs"


def bf16_out(ref, tol):
    """Bound of a result stored as bf16: one more rounding to nearest even."""
    return tol + UB * (ref.abs() + tol)


def put(t, bf16=False, vm=False):
    """Device copy of host fp32 ``t`` in the requested storage (``ops.cast``) and layout (``ops.to_vm``)."""
    d = t.to(DEV).contiguous()
    if bf16:
        d = ops.cast(d, torch.empty(d.shape, dtype=BF, device=DEV))
    return ops.to_vm(d) if vm else d


def nan_out(shape, bf16=False, vm=False):
    """An output pre-filled with NaN in the requested storage and layout."""
    dt = BF if bf16 else torch.float32
    t = ops.vm_empty(*shape, dtype=dt, device=DEV) if vm else torch.empty(shape, dtype=dt, device=DEV)
    return t.fill_(NAN)


def nan_ws(nbytes):
    return torch.full((nbytes // 4 + 1,), NAN, dtype=torch.float32, device=DEV)


WORST = {}  # kernel family -> largest err / bound seen in this process (printed per check as well)


def _note(name, worst):
    WORST[name] = max(WORST.get(name, 0.0), worst)


def compare(name, got, ref, tol, shape, exact):
    """``got`` (fp32 or bf16, either layout) against the fp64 ``ref`` (host or device; compared on
    the device): a non-finite element is refused; with ``exact`` the result must EQUAL ref cast to
    fp32 (and rounded to bf16, to nearest even, for a bf16 result), otherwise |got - ref| <= tol
    per element, plus the bf16 rounding of a bf16 result.  Returns max err / bound (0 with
    ``exact``)."""
    assert bool(torch.isfinite(got).all()), (name, shape, "non-finite element (left unwritten?)")
    g, ref = got.contiguous(), ref.to(got.device)
    if exact:
        want = ref.to(torch.float32)
        if got.dtype == BF:
            want = want.to(BF)
        if not torch.equal(g, want):
            bad = g != want
            raise AssertionError((name, shape, "not exact", int(bad.sum()),
                                  float((g.double() - want.double()).abs().max())))
        return 0.0
    tol = tol.to(got.device)
    if got.dtype == BF:
        tol = bf16_out(ref, tol)
    err = (g.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name} {shape}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}")
    _note(name, worst)
    bad = err > tol
    assert not bool(bad.any()), (name, shape, float(err.max()), worst, int(bad.sum()))
    return worst


def compare_elu_fwd(name, got, pre, tol, shape, exact):
    """Forward with ELU.  ``exact``: equal where pre >= 0 (exp(0) - 1 = 0); for pre < 0 the kernels
    compute fl(exp(pre)) - 1, whose subtraction is exact (Sterbenz for a result above -1/2, a
    result in [-1, -1/2] otherwise) and whose error is therefore that of exp(pre) in (0, 1): one
    unit in the last place of fp32 there, 2^-24 below 1/2 ... 2^-23 at 1, taken as 2^-23 absolute
    -- and for a bf16 result one bf16 unit in the last place of the reference on top of it."""
    pre = pre.to(got.device)
    ref = torch.where(pre > 0, pre, torch.expm1(pre))
    if not exact:
        return compare(name, got, ref, tol.to(got.device) + U * ref.abs().clamp_min(1.0), shape, False)
    assert bool(torch.isfinite(got).all()), (name, shape, "non-finite element (left unwritten?)")
    pos = pre >= 0
    g = got.contiguous()
    want = ref.to(torch.float32).to(got.dtype)
    assert torch.equal(g[pos], want[pos]), (name, shape, "not exact where pre >= 0")
    err = (g.double() - ref).abs()[~pos]
    lim = torch.full_like(err, 2.0 ** -23)
    if got.dtype == BF:
        lim = lim + 2.0 ** (torch.floor(torch.log2(ref[~pos].abs())) - 7)
    worst = float((err / lim).max()) if err.numel() else 0.0
    print(f"{name} {shape}: ELU branch max err {float(err.max()) if err.numel() else 0.0:.3e}, "
          f"max err/ulp {worst:.3f}")
    _note(name + " (exact inputs, err/ulp)", worst)
    assert bool((err <= lim).all()), (name, shape, worst)
    return worst


def check(name, got, ref, tol, shape):
    """Asserts |got - ref| <= tol per element; returns (and prints) max err / bound."""
    err = (got.double().cpu() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name} {shape}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}")
    bad = err > tol
    assert not bool(bad.any()), (name, shape, float(err.max()), worst, int(bad.sum()))
    return worst


def run_kernels(c, general=False):
    """Every product of case ``c`` through ops (the general family where the
    shape has no instance, or everywhere with ``general``)."""
    batch, vsrc, rows, seq, cin, cout = c.shape
    d, kw = c.d, {"general": True} if general else {}
    out = {}
    out["y_none"] = ops.spiral_conv_fwd(d["x"], d["idx"], d["w"], d["b"], ACT_NONE, **kw)
    out["y_elu"] = ops.spiral_conv_fwd(d["x"], d["idx"], d["w"], d["b"], ACT_ELU, **kw)
    out["dx"] = ops.spiral_conv_bwd_data(d["dpre"], c.inv, d["w"], vsrc, **kw)
    out["dx_elu"] = ops.spiral_conv_bwd_data(d["dpre"], c.inv, d["w"], vsrc, elu_y=d["elu_y"], **kw)
    need = ops.spiral_conv_bwd_weight_workspace(batch, rows, seq, cin, cout, **kw)
    assert need > 0
    ws = torch.empty(need // 4, dtype=torch.float32, device=DEV)
    out["dw"], out["db"] = torch.empty_like(d["w"]), torch.empty_like(d["b"])
    assert ops.spiral_conv_bwd_weight(d["x"], d["idx"], d["dpre"], out["dw"], out["db"], ws, **kw) is None
    return out, ws


def check_case(c, out):
    s = c.shape
    tol = gamma(c.n_fwd) * c.pre_abs
    check("fwd", out["y_none"], c.pre, tol, s)
    ref = torch.where(c.pre > 0, c.pre, torch.expm1(c.pre))
    check("fwd+elu", out["y_elu"], ref, tol + U * ref.abs().clamp_min(1.0), s)
    tol = gamma(c.n_dx) * c.dx_abs
    check("dx", out["dx"], c.dx, tol, s)
    ref = c.g * c.dx
    check("dx*elu'", out["dx_elu"], ref, c.g * tol + U * (ref.abs() + c.g * tol), s)
    check("dw", out["dw"], c.dw, gamma(c.n_dw) * c.dw_abs, s)
    check("db", out["db"], c.db, gamma(c.n_dw) * c.db_abs, s)


# ------------------------------------------------------------------ the vertex-major / bf16 tests' cases
SEQ = 9
CHUNK = 4096  # rows per step of the fp64 restatement
TABLES = {"random": spiral_tables.random, "hubs": spiral_tables.hubs, "head_edge": spiral_tables.head_edge,
          "one_vertex_rows": spiral_tables.one_vertex_rows}


@contextlib.contextmanager
def host_threads():
    """The fp64 restatement on every core the run may use (other test modules set one thread)."""
    before = torch.get_num_threads()
    torch.set_num_threads(max(before, min(16, int(os.environ.get("OMP_NUM_THREADS", "8")))))
    try:
        yield
    finally:
        torch.set_num_threads(before)


def make_conv_case(batch, vsrc, rows, cin, cout, table, values, fan=None, dpre_values=exact_values.DYADIC,
                   bf16=(), inverse_bf16=False, device=DEV, parts=exact_values.ALL_PARTS):
    """A case on a synthetic table (``table`` a name of TABLES, or "fan" with ``fan``) in the exact
    or the randn mode, ``elu_edges`` set.  Exact: the conditions of ``exact_values`` are asserted
    (``inverse_bf16``: with the bf16 round trip of the per-slot list sums).  ``c.flat`` is the
    (table, width) pair of ``topology.inverse_flat`` up to width 20 where the fan-in allows one."""
    if table == "fan":
        idx = spiral_tables.fan_table(rows, vsrc, fan, seed=fan + cout)
    else:
        idx = TABLES[table](rows, vsrc, seed=1)
    with host_threads():
        c = Case(batch, vsrc, rows, SEQ, cin, cout, seed=exact_values.seed_of(batch, vsrc, rows, cin, cout), idx=idx,
                 chunk=CHUNK, elu_edges=True, values=values, dpre_values=dpre_values, bf16=bf16, device=device,
                 parts=parts)
        if c.exact:
            c.margins = exact_values.assert_exact(c.ref, (c.idx, c.dpre, vsrc) if inverse_bf16 else None)
    if table in ("head_edge", "fan"):
        assert bool(c.absent_all[0]) and bool(c.absent_all[vsrc - 1])
    c.g0 = c.elu_y == -1.0
    assert bool(c.g0.any()) and bool((c.elu_y == 0.0).any())
    c.flat = None
    if device is not None:
        c.g0 = c.g0.to(device)
        flat, width = topology.inverse_flat(idx, vsrc, max_width=20)
        if flat is not None:
            c.flat = (torch.from_numpy(flat).to(device), width)
    return c


def assert_exact_zeros(c, dx, with_elu):
    """dx of a vertex in no spiral, and under ELU' = 0, is exactly 0."""
    dx = dx.contiguous()
    assert torch.count_nonzero(dx[:, c.absent_all.to(dx.device)]) == 0
    if with_elu:
        assert torch.count_nonzero(dx[c.g0]) == 0


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous(), b.contiguous())
