"""Case builder shared by the SpiralConv kernel tests (``test_gpu_general_conv``,
``test_gpu_specialised_conv``): the inputs of one conv, its fp64 restatement
(index_select + matmul; dx by index_add_; dW by G^T.dY) and the per-element
bounds derived in ``test_gpu_general_conv``'s docstring.  A plain module, no
fixtures: importing it loads libcfsd."""
import numpy as np
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import ops, topology  # noqa: E402
from craniofacialsd_vae_amd.ops import ACT_ELU, ACT_NONE  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


class Case:
    """Inputs of one conv (host fp32 + device copies) and its fp64 restatement.

    ``idx``: a ready ``[rows, seq]`` index table (``spiral_tables``) instead of
    the draw with replacement; every vertex it leaves out is in ``absent_all``.
    ``chunk``: rows per step of the restatement (the gathered ``[batch, rows,
    seq * cin]`` fp64 operand then exists for ``chunk`` rows at a time); the
    sums are fp64 either way.  ``elu_edges``: some ``elu_y`` entries are set to
    exactly -1 (ELU' = 0) and exactly 0."""

    def __init__(self, batch, vsrc, rows, seq, cin, cout, seed, idx=None, chunk=None, elu_edges=False):
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
        self.x = torch.randn(batch, vsrc, cin, generator=g)
        self.w = torch.randn(cout, seq * cin, generator=g)
        self.b = torch.randn(cout, generator=g)
        self.dpre = torch.randn(batch, rows, cout, generator=g)
        # ELU outputs as the forward kernels produce them: fl(fl(exp(v)) - 1) for v <= 0
        v = torch.randn(batch, vsrc, cin, generator=g)
        self.elu_y = torch.where(v > 0, v, torch.exp(v) - 1.0)
        if elu_edges:
            self.elu_y[:, 0::5, 0::3] = -1.0  # exp underflowed: g = 0
            self.elu_y[:, 1::5, 0::3] = 0.0   # v = 0: g = 1
        inv = topology.inverse_spiral(idx.numpy(), vsrc)
        self.d = {k: getattr(self, k).to(DEV) for k in ("x", "w", "b", "dpre", "elu_y")}
        self.d["idx"] = idx.to(torch.int32).to(DEV)
        self.inv = tuple(torch.from_numpy(a).to(DEV) for a in inv)
        self._ref(chunk)

    def _ref(self, chunk=None):
        batch, vsrc, rows, seq, cin, cout = self.shape
        x, w, b, dp = self.x.double(), self.w.double(), self.b.double(), self.dpre.double()
        chunk = rows if chunk is None else chunk
        pre, pre_abs = [], []
        self.dx = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
        self.dx_abs = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
        self.dw = torch.zeros(cout, seq * cin, dtype=torch.float64)
        self.dw_abs = torch.zeros(cout, seq * cin, dtype=torch.float64)
        for r0 in range(0, rows, chunk):
            r1 = min(r0 + chunk, rows)
            flat = self.idx[r0:r1].reshape(-1)
            G = x[:, flat].reshape(batch, r1 - r0, seq * cin)
            pre.append(G @ w.T + b)
            pre_abs.append(G.abs() @ w.abs().T + b.abs())
            dpc = dp[:, r0:r1]
            dG = (dpc @ w).reshape(batch, (r1 - r0) * seq, cin)
            dG_abs = (dpc.abs() @ w.abs()).reshape(batch, (r1 - r0) * seq, cin)
            self.dx.index_add_(1, flat, dG)
            self.dx_abs.index_add_(1, flat, dG_abs)
            G2, dp2 = G.reshape(batch * (r1 - r0), -1), dpc.reshape(batch * (r1 - r0), cout)
            self.dw += dp2.T @ G2
            self.dw_abs += dp2.abs().T @ G2.abs()
        self.pre = pre[0] if len(pre) == 1 else torch.cat(pre, 1)
        self.pre_abs = pre_abs[0] if len(pre_abs) == 1 else torch.cat(pre_abs, 1)
        self.n_fwd = seq * cin + 1
        self.n_dx = (torch.bincount(self.idx.reshape(-1), minlength=vsrc) * cout).double().view(1, vsrc, 1)
        y = self.elu_y.double()
        self.g = torch.where(y > 0, torch.ones_like(y), y + 1)
        dp2 = dp.reshape(batch * rows, cout)
        self.db, self.db_abs = dp2.sum(0), dp2.abs().sum(0)
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
