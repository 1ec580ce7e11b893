"""The step-end kernels of train_ops.hip against float64 autograd (needs an MI355X):
recon_lap_fwd_k / recon_lap_bwd_k, loss_finalize_block, latent_body (behind
cfsd_latent_fwd and cfsd_latent_linear_fwd), latent_bwd_k and phase L of
bottleneck_bwd_k.

Error measure: ``err_rel_max(got, ref) = max|got - ref| / max|ref|``, applied PER
OUTPUT BLOCK (each third of dlat, each half of dmulv, unit, dpred, each loss) --
never ``1 + max|ref|`` and never over blocks of different magnitude, which is how a
1e-4-weighted KL gradient hides behind an O(1) neighbour.

Tolerance of the fp32 kernel against the float64 reference: the project's 1e-5 for
every block.  A block would take 4 x the CPU float32 error of its own reference
expression instead if that error exceeded 2.5e-6; measured for every block checked
here (same inputs, the reference functions below run with dtype=float32), none does.
The largest per group: recon/Laplacian unit 1.3e-6 (16 x 4100 x 3), dpred 1.5e-7,
rec / lap 7.3e-8; latent forward dLC/dz 1.7e-7 (the hinge gradient sums), the
KL thirds 1.2e-7, z / kl / lc 1.8e-7, fused Linear out 5.8e-8; latent backward dmu /
dlogvar 1.7e-7 (sigmoid AE), 1.6e-7 with 17 / 18 parts; bottleneck dmu 3.3e-7, dlogvar
5.1e-7.  No tolerance here comes from what a kernel returned.
"""
import functools

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe
import synthetic_topology as ST
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import engine as E  # noqa: E402
from craniofacialsd_vae_amd import ops, topology  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ETA1, ETA2 = 0.3, 0.8

TOL = 1e-5  # every block (module docstring)


def err_rel_max(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def check(group, case, block, got, ref, tag=""):
    """One block against its float64 reference, the figure printed before the assertion."""
    err = err_rel_max(got, ref)
    print(f"{group} {case}{tag} {block}: err_rel_max {err:.3e}")
    assert err <= TOL, f"{group} {case}{tag} {block}: err_rel_max {err:.3e} > {TOL:.0e}"


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ------------------------------------------------------------ 1. recon + Laplacian
# (B, nv, C): one workgroup that is first and last; 771 rows (3 in the last workgroup); every
# channel count; 257 partial pairs (the finalise loop's second stride).
RL_CASES = [(1, 5, 3), (3, 257, 3), (2, 300, 1), (5, 131, 2), (4, 200, 4), (16, 4100, 3)]
RL_W = (0.7, 0.3)                                  # (w_rec, w_lap)
RL_TERMS, RL_WKL, RL_WLC = (0.37, 1.9), 0.25, 0.6  # kl, lc and their weights: no two equal
TINY_ROW, TINY = 2, 1e-30                          # the Laplacian row whose squared norm underflows


@functools.lru_cache(maxsize=None)
def make_laplacian(nv):
    """A random NON-symmetric COO (row, col, val, (nv, nv)) in shuffled order with row degrees
    0, 1, 7, 8, 9, 16, 17 (lap_row_dot's chunks of 8), duplicate (row, col) entries, and three
    rows whose norm is zero in fp32 (``make_fields`` sets the vertices they read):
    row 0 has no entry; row 1 = (-1, 0.5, 0.5) over the last three vertices, where pred = 1.0
    (product exactly zero in fp32 and fp64); row 2 = one weight 1.0 onto vertex nv - 4, where
    pred = 1e-30: L.pred = 1e-30 is a normal fp32 number whose square underflows to 0.  No
    other row reads vertex nv - 4."""
    rs = np.random.RandomState(1000 + nv)
    degs = [0, 3, 1] + [(7, 8, 9, 16, 17, 1, 2, 5)[i % 8] for i in range(nv - 3)]
    others = np.delete(np.arange(nv), nv - 4)
    row, col, val = [], [], []
    for r, d in enumerate(degs):
        if r == 1:
            cols, vals = np.arange(nv - 3, nv), np.array([-1.0, 0.5, 0.5])
        elif r == TINY_ROW:
            cols, vals = np.array([nv - 4]), np.array([1.0])
        else:
            cols = rs.choice(others, min(d, nv - 1), replace=False)
            vals = rs.randn(len(cols))
        row += [r] * len(cols)
        col += list(cols)
        val += list(vals)
    row, col, val = np.array(row), np.array(col), np.array(val)
    dup = rs.choice(np.flatnonzero((row != 1) & (row != TINY_ROW)), max(2, nv // 16), replace=False)
    row, col = np.concatenate([row, row[dup]]), np.concatenate([col, col[dup]])
    val = np.concatenate([val, rs.randn(len(dup))]).astype(np.float32)
    order = rs.permutation(len(row))
    row, col, val = row[order].astype(np.int64), col[order].astype(np.int64), val[order]
    pairs = set(zip(row.tolist(), col.tolist()))
    assert len(pairs) < len(row), "no duplicate entry"
    assert any((c, r) not in pairs for r, c in pairs), "symmetric pattern"
    deg = np.bincount(np.array(sorted(pairs))[:, 0], minlength=nv)
    want = {0, 1, 7, 8, 9, 16, 17} if nv > 17 else {0, 1, min(nv - 1, 7)}
    assert want <= set(deg.tolist()), f"row degrees {sorted(set(deg.tolist()))}"
    return row, col, val, (nv, nv)


def device_csr(lap):
    """CSR and transposed CSR as DeviceTopology makes them (coalesce, then group by row / column)."""
    row, col, val, (nv, _) = lap
    r, c, v = topology.coalesced_csr(row, col, val, nv)
    assert len(r) < len(row)
    dev = lambda t: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in t)  # noqa: E731
    return dev(topology.csr_from_coo(r, c, v, nv)), dev(topology.csr_transpose_from_coo(r, c, v, nv))


def make_fields(B, nv, C, seed=0):
    g = torch.Generator().manual_seed(17 * B + nv + C + 1000 * seed)
    pred, gt = torch.randn(B, nv, C, generator=g), torch.randn(B, nv, C, generator=g)
    pred[:, nv - 3:, :] = 1.0
    pred[:, nv - 4, :] = TINY
    return pred, gt


def lap_apply(pred, lap):
    row, col, val, shape = lap
    L = torch.sparse_coo_tensor(torch.as_tensor(np.stack([row, col])), torch.as_tensor(val), shape)
    b, n = pred.shape[0], pred.shape[1]
    return L.mm(pred.transpose(0, 1).reshape(n, -1)).reshape(n, b, -1).transpose(1, 0)


def recon_lap_reference(pred, gt, lap, w_rec, w_lap, dtype=F64):
    """Losses by the oracle, dpred by autograd of w_rec * mse + w_lap * lap, unit = Lx / |Lx|
    (0 where |Lx| == 0; torch.norm's gradient at an exactly zero row is 0, the kernel's branch).

    Row TINY_ROW is left out of the reference's Laplacian: its L.pred = 1e-30 has a squared norm
    that underflows in fp32, so the kernel's sqrtf(sum of squares) is 0: unit 0 and no gradient,
    where float64 would see a true unit vector.  What the row adds to the loss (1e-30)
    is far below the tolerance."""
    row, col, val, shape = lap
    keep = row != TINY_ROW
    assert keep.sum() == len(row) - 1 and float(pred[:, col[~keep]].abs().max()) == np.float32(TINY)
    lap = (row[keep], col[keep], val[keep].astype(np.float64 if dtype == F64 else np.float32), shape)
    p = pred.to(dtype).clone().requires_grad_()
    rec, lp = O.mse_loss(p, gt.to(dtype)), O.laplacian_loss(p, lap)
    (dpred,) = torch.autograd.grad(w_rec * rec + w_lap * lp, p)
    with torch.no_grad():
        lx = lap_apply(p, lap)
        nrm = lx.norm(dim=-1, keepdim=True)
        unit = torch.where(nrm > 0, lx / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(lx))
    assert bool((nrm[:, 1] == 0).all()), "row 1 is the exactly-zero row"
    assert torch.isfinite(dpred).all()
    return {"unit": unit, "dpred": dpred, "rec": rec.detach(), "lap": lp.detach()}


@functools.lru_cache(maxsize=None)
def rl_case(B, nv, C, w=RL_W):
    lap = make_laplacian(nv)
    pred, gt = make_fields(B, nv, C)
    return lap, pred, gt, recon_lap_reference(pred, gt, lap, *w)


def run_recon_lap(pred, gt, csr, csrT, w, vm, fused, acc=None, terms=RL_TERMS):
    """recon_lap_fwd, then the gradient and the loss reduction in one launch (``fused``) or two."""
    B, nv, C = pred.shape
    lay = ops.to_vm if vm else (lambda t: t)
    p, g = lay(pred.to(DEV)), lay(gt.to(DEV))
    unit, dpred = lay(nan(B, nv, C)), lay(nan(B, nv, C))
    assert ops.is_vm(unit) == (vm and B > 1)
    partials, out = nan(2 * ops.recon_lap_blocks(B, nv)), nan(5)
    t = torch.tensor(terms, device=DEV)
    ops.recon_lap_fwd(p, g, csr, unit, partials)
    if fused:
        ops.recon_lap_bwd_finalize(p, g, unit, csrT, dpred, w[0], w[1], partials, t, out, acc, RL_WKL, RL_WLC)
    else:
        ops.recon_lap_bwd(p, g, unit, csrT, dpred, w[0], w[1])
        ops.loss_finalize(partials, t, out, acc, B, nv, C, RL_WKL, RL_WLC, w[1])
    return unit.cpu(), dpred.cpu(), out.cpu()


def check_zero_rows(case, tag, unit, dpred, pred, gt, w_rec):
    """Rows 0, 1 and TINY_ROW have norm 0 in fp32: unit exactly 0 (the underflowing row's
    L.pred is NOT 0: a branch value other than 0 would show as unit = 1e-30), and vertex nv - 4,
    read by that row alone, gets the MSE gradient alone."""
    B, nv, C = pred.shape
    assert bool((unit[:, :TINY_ROW + 1] == 0).all()), "degree-0, zero-product and underflowing row: unit is 0"
    got = dpred[:, nv - 4]
    assert torch.isfinite(got).all()
    mse = 2.0 * w_rec / (B * nv * C) * (pred[:, nv - 4].double() - gt[:, nv - 4].double())
    if w_rec:
        check("recon_lap", case, "dpred[nv-4]", got, mse, tag)
    else:
        assert bool((got == 0).all())


def check_losses(case, tag, out, ref, w_lap, terms=RL_TERMS):
    check("recon_lap", case, "rec", out[0], ref["rec"], tag)
    check("recon_lap", case, "lap", out[3], ref["lap"], tag)
    t = np.array(terms, np.float32)
    assert out[1].item() == t[0] and out[2].item() == t[1], "kl / lc are passed through"
    # tot = rec + w_kl kl + w_lc lc + w_lap lap over the kernel's own fp32 terms, all positive:
    # three products and three sums (or fused multiply-adds) of at most 2^-24 relative error each
    o = out.double().numpy()
    tot = o[0] + np.float32(RL_WKL).astype(np.float64) * o[1] + np.float32(RL_WLC).astype(np.float64) * o[2] \
        + np.float32(w_lap).astype(np.float64) * o[3]
    err = abs(o[4] - tot) / tot
    print(f"recon_lap {case}{tag} tot: rel {err:.3e}")
    assert err <= 6 * 2.0 ** -24


@pytest.mark.parametrize("B,nv,C", RL_CASES)
def test_recon_lap_vs_float64(B, nv, C):
    """unit, dpred, rec and lap against float64 in both layouts; vertex-major bit-equal to
    batch-major; the one-launch gradient + finalise bit-equal to the two launches.

    Rows 0 (no entry), 1 (product exactly zero) and 2 (L.pred = 1e-30, squared norm underflows)
    take recon_lap_fwd_k's ``nrm > 0 ? 1 / nrm : 0`` branch: their unit vectors are exactly 0 and
    no NaN reaches dpred (an unguarded 1 / nrm gives 0 * inf).  Row 2 shows the branch's VALUE:
    anything but 0 there leaves unit = value * 1e-30 != 0 (``check_zero_rows``)."""
    lap, pred, gt, ref = rl_case(B, nv, C)
    csr, csrT = device_csr(lap)
    case = f"{B}x{nv}x{C}"
    res = {}
    for vm in (False, True):
        for fused in (True, False):
            unit, dpred, out = res[vm, fused] = run_recon_lap(pred, gt, csr, csrT, RL_W, vm, fused)
            tag = ("-vm" if vm else "-bm") + ("-fused" if fused else "")
            check("recon_lap", case, "unit", unit, ref["unit"], tag)
            check("recon_lap", case, "dpred", dpred, ref["dpred"], tag)
            check_losses(case, tag, out, ref, RL_W[1])
            check_zero_rows(case, tag, unit, dpred, pred, gt, RL_W[0])
        for a, b, what in zip(res[vm, True], res[vm, False], ("unit", "dpred", "losses")):
            assert torch.equal(a, b), f"one launch vs two, {what}, vm={vm}"
    for a, b, what in zip(res[False, True], res[True, True], ("unit", "dpred")):
        assert torch.equal(a, b), f"vertex-major vs batch-major {what}"


@pytest.mark.parametrize("w", [(1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("vm", [False, True])
def test_recon_lap_each_term_alone(w, vm):
    B, nv, C = 3, 257, 3
    lap, pred, gt, _ = rl_case(B, nv, C)
    ref = recon_lap_reference(pred, gt, lap, *w)
    csr, csrT = device_csr(lap)
    unit, dpred, out = run_recon_lap(pred, gt, csr, csrT, w, vm, True)
    case, tag = f"{B}x{nv}x{C}-w{w[0]:g}/{w[1]:g}", "-vm" if vm else "-bm"
    check("recon_lap", case, "unit", unit, ref["unit"], tag)
    check("recon_lap", case, "dpred", dpred, ref["dpred"], tag)
    check_losses(case, tag, out, ref, w[1])
    check_zero_rows(case, tag, unit, dpred, pred, gt, w[0])


@pytest.mark.parametrize("fused", [True, False])
def test_loss_accumulator(fused):
    """Three calls on different inputs: acc[0:5] is the sum of the three ``out`` vectors in call
    order (bit for bit against the same fp32 additions on the host), acc[5] == 3; without ``acc``
    nothing else changes."""
    B, nv, C = 3, 257, 3
    lap = make_laplacian(nv)
    csr, csrT = device_csr(lap)
    acc = torch.zeros(6, device=DEV)
    host = np.zeros(5, np.float32)
    for i in range(3):
        pred, gt = make_fields(B, nv, C, seed=i)
        terms = (0.37 + i, 1.9 / (1 + i))
        _, dpred, out = run_recon_lap(pred, gt, csr, csrT, RL_W, False, fused, acc=acc, terms=terms)
        _, dpred0, out0 = run_recon_lap(pred, gt, csr, csrT, RL_W, False, fused, acc=None, terms=terms)
        assert torch.equal(dpred, dpred0) and torch.equal(out, out0)
        host = host + out.numpy()
        assert host.dtype == np.float32
    got = acc.cpu().numpy()
    assert np.array_equal(got[:5], host), (got, host)
    assert got[5] == 3.0


def test_recon_lap_refuses_bad_operands():
    """C = 5, B = 0 and a null operand raise through ops and launch nothing."""
    nv = 131
    csr, csrT = device_csr(make_laplacian(nv))
    outputs = ("unit", "dpred", "partials", "out", "acc")

    def operands(B, C):
        seven = lambda *s: torch.full(s, 7.0, device=DEV)  # noqa: E731
        return dict(pred=torch.ones(B, nv, C, device=DEV), gt=torch.ones(B, nv, C, device=DEV),
                    unit=seven(B, nv, C), dpred=seven(B, nv, C), partials=seven(2 * ops.recon_lap_blocks(B, nv)),
                    out=seven(5), acc=seven(6), terms=torch.tensor(RL_TERMS, device=DEV), l_col=csr[1],
                    lt_val=csrT[2])

    def calls(a):
        L, LT = (csr[0], a["l_col"], csr[2]), (csrT[0], csrT[1], a["lt_val"])
        return {"fwd": lambda: ops.recon_lap_fwd(a["pred"], a["gt"], L, a["unit"], a["partials"]),
                "bwd": lambda: ops.recon_lap_bwd(a["pred"], a["gt"], a["unit"], LT, a["dpred"], *RL_W),
                "fin": lambda: ops.recon_lap_bwd_finalize(a["pred"], a["gt"], a["unit"], LT, a["dpred"], *RL_W,
                                                          a["partials"], a["terms"], a["out"], a["acc"], RL_WKL,
                                                          RL_WLC)}

    def refused(a, which, kept):
        for name in which:
            with pytest.raises((ValueError, RuntimeError)):
                calls(a)[name]()
        torch.cuda.synchronize()
        for k in outputs:
            assert bool((kept[k] == 7.0).all()), f"{k} was written"

    for B, C in ((2, 5), (0, 3)):
        a = operands(B, C)
        refused(a, ("fwd", "bwd", "fin"), a)
    for null, which in (("unit", ("fwd", "bwd", "fin")), ("partials", ("fwd", "fin")), ("l_col", ("fwd",)),
                        ("lt_val", ("bwd", "fin")), ("dpred", ("bwd", "fin")), ("terms", ("fin",)),
                        ("out", ("fin",))):
        kept = operands(2, 3)
        refused(dict(kept, **{null: None}), which, kept)


# ------------------------------------------------------------ 2. latent head, forward
class Lat:
    """One latent-head case.  mu = s_mu * randn, logvar = 0.3 * randn, eps = s_eps * randn: the
    scales and the seed were chosen on the CPU so that the float64 reference meets the hinge
    conditions asserted in ``latent_reference``."""

    def __init__(self, name, bs, L, nreg=15, key=0, vae=True, train=True, sigmoid=False, w_kl=1e-4, w_lc=0.5,
                 B=None, s_mu=0.15, s_eps=0.2, seed=0):
        self.name, self.bs, self.L, self.nreg, self.key = name, bs, L, nreg, key
        self.vae, self.train, self.sigmoid, self.w_kl, self.w_lc = vae, train, sigmoid, w_kl, w_lc
        self.B = bs * bs if B is None else B
        self.s_mu, self.s_eps, self.seed = s_mu, s_eps, seed
        self.rs = L // nreg
        self.region = O.latent_regions(nreg, L)[key]


LAT_CASES = [
    Lat("vae-k0", 4, 75, key=0),
    Lat("vae-k14", 4, 75, key=14, seed=1),
    Lat("vae-33", 3, 33, key=14, seed=2),      # region size 2, dimensions 30..32 belong to "the rest"
    Lat("vae-30", 5, 30, nreg=4, key=1),       # region size 7, two left over
    Lat("vae-bs9", 9, 75, key=3),              # 29 KB of dynamic LDS
    Lat("vae-bs16", 16, 75, key=11, seed=34),  # 105 KB: the raised dynamic-LDS limit (> 64 KB)
    Lat("vae-eval", 4, 75, key=7, train=False, s_mu=0.2),
    Lat("ae", 4, 33, key=5, vae=False, w_kl=0.0, s_mu=0.2, seed=18),
    Lat("ae-sigmoid", 4, 33, key=5, vae=False, sigmoid=True, w_kl=0.0, s_mu=3.0),
    Lat("no-lc", None, 75, w_lc=0.0, B=6),
    Lat("kl-256", None, 75, w_lc=0.0, B=256),  # the KL gradient alone at its 1e-4 / 256 scale (section 3)
    Lat("kl-1", 4, 75, key=2, w_kl=1.0, seed=2),
]
LAT = {c.name: c for c in LAT_CASES}


def hinge_args(z, region, bs, eta1, eta2):
    """The two hinge families' arguments of O.latent_consistency (lg - dg + eta1, lr - dr + eta2)."""
    a, b = region
    zf = z[:, a:b].reshape(bs, bs, -1)
    ze = torch.cat([z[:, :a], z[:, b:]], dim=1).reshape(bs, bs, -1)
    p, q = torch.triu_indices(bs, bs, 1)
    lg = ((zf[q] - zf[p]) ** 2).sum(-1).reshape(-1)
    dg = ((zf[:, q].transpose(0, 1) - zf[:, p].transpose(0, 1)) ** 2).sum(-1).reshape(-1)
    dr = ((ze[q] - ze[p]) ** 2).sum(-1).reshape(-1)
    lr = ((ze[:, q].transpose(0, 1) - ze[:, p].transpose(0, 1)) ** 2).sum(-1).reshape(-1)
    return lg - dg + eta1, lr - dr + eta2


@functools.lru_cache(maxsize=None)
def latent_inputs(name):
    c = LAT[name]
    g = torch.Generator().manual_seed(c.seed)
    mu = c.s_mu * torch.randn(c.B, c.L, generator=g)
    lv = 0.3 * torch.randn(c.B, c.L, generator=g)
    eps = c.s_eps * torch.randn(c.B, c.L, generator=g)
    G = torch.randn(c.B, c.L, generator=g)
    return {"mu": mu, "lv": lv, "eps": eps, "G": G, "mulv": torch.cat([lv, mu], 1) if c.vae else mu.clone()}


def latent_reference(c, inp, dtype=F64, G=None, w_kl=None, w_lc=None):
    """z, kl, lc and the three thirds of dlat, each third from its own autograd.grad call; with
    ``G`` also dmu / dlogvar of sum(z * G) + w_kl * kl + w_lc * lc (for the sigmoid AE with
    respect to the pre-sigmoid mu).

    The hinge conditions are asserted here, on the float64 reference: in each family between
    20 % and 80 % of the terms are active and no argument is closer to 0 than 1e-3.  At exactly
    0 ``torch.clamp`` passes gradient and the kernel's ``> 0`` does not: ties are not under test."""
    w_kl = c.w_kl if w_kl is None else w_kl
    w_lc = c.w_lc if w_lc is None else w_lc
    mu = inp["mu"].to(dtype).clone().requires_grad_()
    lv = inp["lv"].to(dtype).clone().requires_grad_()
    if c.vae:
        z = mu + inp["eps"].to(dtype) * torch.exp(0.5 * lv) if c.train else mu.clone()
    else:
        z = torch.sigmoid(mu) if c.sigmoid else mu.clone()
    zero = torch.zeros((), dtype=dtype)
    kl = O.kl_loss(mu, lv) if c.vae else zero
    r = {"z": z.detach(), "kl": kl.detach(), "lc": zero, "d_lc": torch.zeros_like(mu),
         "d_kl_mu": torch.zeros_like(mu), "d_kl_lv": torch.zeros_like(mu)}
    lc = zero
    if w_lc:
        lc = O.latent_consistency(z, c.region, c.bs, ETA1, ETA2)
        r["lc"] = lc.detach()
        r["d_lc"] = w_lc * torch.autograd.grad(lc, z, retain_graph=True)[0]
        if dtype == F64:
            scale = 1.0 / (c.bs ** 3 - c.bs ** 2)
            fams = hinge_args(z.detach(), c.region, c.bs, ETA1, ETA2)
            assert abs(scale * sum(f.clamp(min=0).sum() for f in fams) - lc.item()) <= 1e-12 * lc.item()
            for f in fams:
                active = (f > 0).double().mean().item()
                assert 0.2 <= active <= 0.8, f"{c.name}: {active:.0%} of a hinge family active"
                assert f.abs().min().item() >= 1e-3, f"{c.name}: hinge argument {f.abs().min().item():.2e}"
    if c.vae:
        r["d_kl_mu"] = w_kl * torch.autograd.grad(kl, mu, retain_graph=True)[0]
        r["d_kl_lv"] = w_kl * torch.autograd.grad(kl, lv, retain_graph=True)[0]
    if G is not None:
        tot = (z * G.to(dtype)).sum() + w_kl * kl + w_lc * lc
        g = torch.autograd.grad(tot, (mu, lv) if c.vae else (mu,), allow_unused=True)
        r["dmu"] = g[0]
        if c.vae:
            r["dlv"] = g[1] if g[1] is not None else torch.zeros_like(mu)
    return r


@functools.lru_cache(maxsize=None)
def lat_ref(name):
    return latent_reference(LAT[name], latent_inputs(name), G=latent_inputs(name)["G"])


def run_latent_fwd(c, inp, linear=None, w_kl=None, w_lc=None):
    w_kl = c.w_kl if w_kl is None else w_kl
    w_lc = c.w_lc if w_lc is None else w_lc
    z, dlat, terms = nan(c.B, c.L), nan(c.B, 3 * c.L), nan(2)
    eps = inp["eps"].to(DEV) if (c.vae and c.train) else None
    key = torch.tensor([c.key], dtype=torch.int32, device=DEV) if w_lc else None
    args = (inp["mulv"].to(DEV), eps, key, z, dlat, terms, c.L, c.rs if w_lc else 0, c.train, c.vae, c.sigmoid,
            w_kl, w_lc, ETA1, ETA2)
    if linear is None:
        ops.latent_fwd(*args)
        return z, dlat, terms
    W, bias = linear
    y = nan(c.B, W.shape[0])
    assert ops.latent_linear_fwd_supported(c.B, c.L, W.shape[0])
    ops.latent_linear_fwd(*args, W.to(DEV), bias.to(DEV), y)
    return z, dlat, terms, y


def check_latent_fwd(c, ref, z, dlat, terms):
    L = c.L
    check("latent_fwd", c.name, "z", z, ref["z"])
    thirds = (("d_lc", dlat[:, :L], c.w_lc != 0), ("d_kl_mu", dlat[:, L:2 * L], c.vae),
              ("d_kl_lv", dlat[:, 2 * L:], c.vae))
    for block, got, live in thirds:
        if live:
            check("latent_fwd", c.name, block, got, ref[block])
        else:
            assert bool((got == 0).all()), f"{c.name}: {block} must be exactly 0"
    for block, got, live in (("kl", terms[0], c.vae), ("lc", terms[1], c.w_lc != 0)):
        if live:
            check("latent_fwd", c.name, block, got, ref[block])
        else:
            assert got.item() == 0.0, f"{c.name}: {block} must be exactly 0"


@pytest.mark.parametrize("name", [c.name for c in LAT_CASES])
def test_latent_fwd_vs_float64(name):
    """z, kl, lc and each third of dlat (w_lc dLC/dz | w_kl dKL/dmu | w_kl dKL/dlogvar) at its own
    scale, with eta1 != eta2.  See ``latent_reference`` for the conditions on the inputs (asserted
    there; at a hinge argument of exactly 0 torch.clamp passes gradient and the kernel's ``> 0``
    does not -- ties are not under test)."""
    c, inp, ref = LAT[name], latent_inputs(name), lat_ref(name)
    z, dlat, terms = run_latent_fwd(c, inp)
    check_latent_fwd(c, ref, z, dlat, terms)
    if not (c.vae and c.train) and not c.sigmoid:
        assert torch.equal(z, inp["mu"].to(DEV)), "z == mu bit for bit"
    if name == "vae-eval":  # KL is reported in eval mode as in train mode (same mulv, train = 1)
        _, _, terms_train = run_latent_fwd(LAT["vae-k0"], inp)
        assert torch.equal(terms[:1], terms_train[:1])


@pytest.mark.parametrize("name", ["vae-k14", "ae-sigmoid"])
def test_latent_linear_fwd(name):
    """The fused head + decoder Linear: z, dlat and terms bit-equal to latent_fwd, out against
    float64 z W^T + b (n = 200: seven 32-column workgroups, the last one of 8 columns)."""
    c, inp, ref = LAT[name], latent_inputs(name), lat_ref(name)
    g = torch.Generator().manual_seed(5)
    W, bias = 0.05 * torch.randn(200, c.L, generator=g), torch.randn(200, generator=g)
    z, dlat, terms, y = run_latent_fwd(c, inp, linear=(W, bias))
    z0, dlat0, terms0 = run_latent_fwd(c, inp)
    assert torch.equal(z, z0) and torch.equal(dlat, dlat0) and torch.equal(terms, terms0)
    check("latent_linear_fwd", name, "out", y, ref["z"] @ W.double().T + bias.double())


# ------------------------------------------------------------ 3. latent head, backward
def run_latent_bwd(c, inp, z, dlat, dz):
    dmulv = nan(*inp["mulv"].shape)
    eps = inp["eps"].to(DEV) if (c.vae and c.train) else None
    ops.latent_bwd(inp["mulv"].to(DEV), eps, z, dz, dlat, dmulv, c.L, c.train, c.vae, c.sigmoid)
    return dmulv


def check_dmulv(group, c, dmulv, ref):
    L = c.L
    if c.vae:
        check(group, c.name, "dlogvar", dmulv[:, :L], ref["dlv"])
        check(group, c.name, "dmu", dmulv[:, L:], ref["dmu"])
    else:
        check(group, c.name, "dmu", dmulv, ref["dmu"])


@pytest.mark.parametrize("name", ["vae-k0", "vae-eval", "ae", "ae-sigmoid"])
def test_latent_bwd_vs_float64(name):
    """dmu / dlogvar with a NONZERO decoder gradient G, against autograd of
    sum(z * G) + w_kl * kl + w_lc * lc."""
    c, inp, ref = LAT[name], latent_inputs(name), lat_ref(name)
    z, dlat, _ = run_latent_fwd(c, inp)
    check_dmulv("latent_bwd", c, run_latent_bwd(c, inp, z, dlat, inp["G"].to(DEV)), ref)


def test_latent_bwd_kl_alone():
    """G = 0 and w_lc = 0: dmulv is the KL gradient alone, at w_kl = 1e-4 and B = 256."""
    c, inp = LAT["kl-256"], latent_inputs("kl-256")
    ref = latent_reference(c, inp, G=torch.zeros(c.B, c.L))
    z, dlat, _ = run_latent_fwd(c, inp)
    check_dmulv("latent_bwd", c, run_latent_bwd(c, inp, z, dlat, torch.zeros(c.B, c.L, device=DEV)), ref)
    assert ref["dlv"].abs().max() < 1e-6, "the scale this case is about"


def test_latent_bwd_reparameterisation_alone():
    """G != 0 and w_kl = w_lc = 0: dmu = G, dlogvar = G eps exp(logvar / 2) / 2."""
    c, inp = LAT["vae-k0"], latent_inputs("vae-k0")
    ref = latent_reference(c, inp, G=inp["G"], w_kl=0.0, w_lc=0.0)
    z, dlat, _ = run_latent_fwd(c, inp, w_kl=0.0, w_lc=0.0)
    assert bool((dlat == 0).all())
    check_dmulv("latent_bwd_reparam", c, run_latent_bwd(c, inp, z, dlat, inp["G"].to(DEV)), ref)


@pytest.mark.parametrize("parts", [1, 2, 17, 18])
def test_latent_bwd_parts(parts):
    """dz_dec as [parts, B, L] partial products (the loads go in batches of 16): against the
    float64 sum, and bit for bit against the parts added in order on the host in fp32."""
    c, inp = LAT["vae-k0"], latent_inputs("vae-k0")
    g = torch.Generator().manual_seed(40 + parts)
    P = torch.randn(parts, c.B, c.L, generator=g)
    ref = latent_reference(c, inp, G=P.double().sum(0))
    z, dlat, _ = run_latent_fwd(c, inp)
    got = run_latent_bwd(c, inp, z, dlat, P.to(DEV))
    check_dmulv("latent_bwd_parts", c, got, ref)
    host = P[0].numpy().copy()
    for p in range(1, parts):
        host = host + P[p].numpy()
    one = run_latent_bwd(c, inp, z, dlat, torch.from_numpy(host).to(DEV))
    assert torch.equal(got, one)


def test_latent_bwd_refuses_missing_operands():
    """The sigmoid AE reads z (zval * (1 - zval)), the training VAE eps: without them the call
    raises before any launch; so do a dlat of the wrong shape and an empty batch."""
    c, inp = LAT["ae-sigmoid"], latent_inputs("ae-sigmoid")
    mulv, dz, dlat = inp["mulv"].to(DEV), inp["G"].to(DEV), torch.zeros(c.B, 3 * c.L, device=DEV)
    dmulv = torch.full_like(mulv, 7.0)
    with pytest.raises((ValueError, RuntimeError)):
        ops.latent_bwd(mulv, None, None, dz, dlat, dmulv, c.L, True, False, True)
    with pytest.raises((ValueError, RuntimeError)):
        ops.latent_bwd(mulv, None, dz, dz, dlat[:, :c.L].contiguous(), dmulv, c.L, True, False, True)
    v, vinp = LAT["vae-k0"], latent_inputs("vae-k0")
    vdm = torch.full((v.B, 2 * v.L), 7.0, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        ops.latent_bwd(vinp["mulv"].to(DEV), None, None, vinp["G"].to(DEV), torch.zeros(v.B, 3 * v.L, device=DEV),
                       vdm, v.L, True, True, False)
    empty = lambda n: torch.empty(0, n, device=DEV)  # noqa: E731
    with pytest.raises((ValueError, RuntimeError)):  # B = 0
        ops.latent_bwd(empty(2 * v.L), empty(v.L), None, empty(v.L), empty(3 * v.L), empty(2 * v.L), v.L, True, True,
                       False)
    torch.cuda.synchronize()
    assert bool((dmulv == 7.0).all()) and bool((vdm == 7.0).all())


# (batch, latent, is_vae, sigmoid, coarse vertices, cup, fine vertices, encoder width)
BN_CASES = [(3, 33, 0, 1, 27, 64, 108, 1728), (5, 16, 1, 0, 80, 64, 320, 1000)]


def bottleneck_reference(B, L, is_vae, sigmoid, up, gfine, wd, mu, lv, eps, dlat, dtype=F64):
    """dmulv of the whole chain: Pool(up)^T of the fine gradient, the decoder Linear's dx, the
    head.  ``dlat``'s thirds enter as the given gradients of z, mu and logvar (linear functionals
    under autograd)."""
    row, col, val, nv = up
    gf = gfine.to(dtype)
    dh = torch.zeros(B, nv, gf.shape[2], dtype=dtype)
    dh.index_add_(1, torch.as_tensor(row), gf[:, torch.as_tensor(col)] * torch.as_tensor(val).to(dtype)[None, :, None])
    dz = dh.reshape(B, -1) @ wd.to(dtype)
    mu = mu.to(dtype).clone().requires_grad_()
    lv = lv.to(dtype).clone().requires_grad_()
    d = dlat.to(dtype)
    if is_vae:
        z = mu + eps.to(dtype) * torch.exp(0.5 * lv)
    else:
        z = torch.sigmoid(mu) if sigmoid else mu.clone()
    tot = (z * (dz + d[:, :L])).sum()
    if is_vae:  # (the AE head reads the first third only)
        tot = tot + (mu * d[:, L:2 * L]).sum() + (lv * d[:, 2 * L:]).sum()
    g = torch.autograd.grad(tot, (mu, lv) if is_vae else (mu,))
    return {"dmu": g[0], "dlv": g[1] if is_vae else None, "z": z.detach()}


def bottleneck_inputs(B, L, is_vae, sigmoid, nv, cup, n_up, ke):
    g = torch.Generator().manual_seed(B * 100 + L)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    row, col, val = [], [], []
    for f in range(n_up):      # a Pool(up)^T-shaped matrix: each fine vertex feeds 3 coarse vertices
        for k in range(3):
            row.append((f * 7 + k * 11) % nv)
            col.append(f)
            val.append(0.1 + 0.3 * k)
    up = (np.array(row), np.array(col), np.array(val, np.float32), nv)
    ne = 2 * L if is_vae else L
    return dict(up=up, gfine=rnd(B, n_up, cup), wd=0.05 * rnd(nv * cup, L), mu=rnd(B, L), lv=0.3 * rnd(B, L),
                eps=rnd(B, L), dlat=rnd(B, 3 * L), xe=rnd(B, ke), we=0.05 * rnd(ne, ke))


@pytest.mark.parametrize("case", BN_CASES, ids=["ae-sigmoid", "vae"])
def test_bottleneck_bwd_dmulv_vs_float64(case):
    """One call of the one-launch bottleneck backward: dmulv (its phase L, fed by the A
    workgroups' partial products) against the float64 chain."""
    B, L, is_vae, sigmoid, nv, cup, n_up, ke = case
    a = bottleneck_inputs(*case)
    row, col, val, _ = a["up"]
    ref = bottleneck_reference(B, L, is_vae, sigmoid, a["up"], a["gfine"], a["wd"], a["mu"], a["lv"], a["eps"],
                               a["dlat"])
    csr = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in topology.csr_from_coo(row, col, val, nv))
    ne, nd = (2 * L if is_vae else L), nv * cup
    mulv = (torch.cat([a["lv"], a["mu"]], 1) if is_vae else a["mu"]).contiguous().to(DEV)
    z = ref["z"].float().to(DEV)  # the sigmoid AE reads it as zval; the decoder Linear's dW is not checked here
    dmulv, sync = nan(B, ne), torch.zeros(ops.BN_SYNC_INTS, dtype=torch.int32, device=DEV)
    xchg = nan(ops.bottleneck_exchange_floats(B, L, nd, ne))
    ops.bottleneck_bwd(csr, a["gfine"].to(DEV), z, a["wd"].to(DEV), xchg, nan(nd, L), nan(nd), mulv,
                       a["eps"].to(DEV), a["dlat"].to(DEV), dmulv, is_vae, sigmoid, a["xe"].to(DEV), a["we"].to(DEV),
                       nan(B, ke), nan(ne, ke), nan(ne), sync)
    torch.cuda.synchronize()
    ops.bottleneck_check(sync)
    assert not sync.any()
    name = "ae-sigmoid" if sigmoid else "vae"
    if is_vae:
        check("bottleneck_bwd", name, "dlogvar", dmulv[:, :L], ref["dlv"])
        check("bottleneck_bwd", name, "dmu", dmulv[:, L:], ref["dmu"])
    else:
        check("bottleneck_bwd", name, "dmu", dmulv, ref["dmu"])


# ------------------------------------------------------------ 4. the sigmoid AE end to end
@pytest.mark.parametrize("eta1,eta2,spread", [(ETA1, ETA2, 1.0), (-0.03, 0.5, 8.0)], ids=["0.3/0.8", "order"])
def test_sigmoid_ae_two_steps_lockstep(eta1, eta2, spread):
    """A plain AE with pre_z_sigmoid and unequal margins, two train steps in lock-step with the
    oracle on the small torus: losses, every gradient, parameters after Adam (the tolerances of
    test_gpu_general_engine.lockstep).

    With margins 0.3 / 0.8 this model's swapped latents lie so close together that every hinge
    term is active: that run pins the margins' sum (1.1, not the default 1.0) and the sigmoid
    path end to end.  The second run pins their ORDER through the engine: the meshes' deviations
    from their mean are spread eightfold and the margins -0.03 / 0.5 (chosen on the CPU) leave
    each hinge family between 20 % and 80 % active in both steps, no argument within 1e-3 of 0
    (asserted on the oracle), so swapped margins would change the loss and every gradient."""
    torch.set_num_threads(4)
    S, out_ch, latent, n_reg = 7, [8, 20], 22, 11
    npz = ST.torus_topology(nu=32, nv=16, factors=(4, 4), seq=S)
    dtopo, otopo = topology.DeviceTopology.from_npz(npz, device=DEV), O.Topology(npz)
    weights = recipe.golden_weights(recipe.param_shapes(num_vert=32, out_ch=out_ch, latent=latent, seq=S,
                                                        is_vae=False), seed=4)
    W = {"kl": 0.0, "lc": 0.5, "lap": 0.1}
    eng = E.SDVAEEngine(dtopo, E.ModelSpec(3, out_ch, latent, is_vae=False, pre_z_sigmoid=True), w_kl=W["kl"],
                        w_lc=W["lc"], w_lap=W["lap"], eta1=eta1, eta2=eta2, swap_bs=4, device=DEV)
    assert eng.spec.sigmoid
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    P = O.make_params(weights)
    opt = O.Adam(P)
    shadow = {k: torch.from_numpy(v.copy()) for k, v in weights.items()}
    shadow_opt = O.Adam(shadow)
    meshes = ST.torus_meshes(8, nu=32, nv=16, seed=2)
    mean = meshes.mean(0, keepdims=True)
    meshes = (mean + spread * (meshes - mean)).astype(np.float32)
    data = torch.from_numpy(meshes).to(DEV)

    def close(a, b, rel, what):
        a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
        err, tol = np.abs(a - b).max(), rel * (1.0 + np.abs(b).max())
        assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"

    for step in range(2):
        key = (2 + 4 * step) % n_reg
        out, grads, x16 = O.train_step(P, opt, meshes[4 * step:4 * step + 4], otopo, key, None, w=W, is_vae=False,
                                       pre_z_sigmoid=True, eta1=eta1, eta2=eta2)
        assert 0 < out["z"].min() and out["z"].max() < 1 and out["lc"].item() > 0
        for f in hinge_args(out["z"].detach().double(), O.latent_regions(n_reg, latent)[key], 4, eta1, eta2):
            active = (f > 0).double().mean().item()
            assert active == 1.0 if spread == 1.0 else 0.2 <= active <= 0.8, f"step {step}: {active:.0%} active"
            assert f.abs().min().item() >= 1e-3
        b = eng.buffers(16)
        b.key.fill_(key)
        b.batch_idx.copy_(torch.arange(4 * step, 4 * step + 4, dtype=torch.int32))
        ops.swap_features(data, b.batch_idx, dtopo.region_mask, b.key, 4, out=b.x)
        eng.train_step_on(b)
        torch.cuda.synchronize()
        assert np.array_equal(b.x.cpu().numpy(), x16.numpy()), f"step {step}: swap differs"
        ref = np.array([out[k].item() for k in ("rec", "kl", "lc", "lap", "tot")])
        np.testing.assert_allclose(b.losses.cpu().numpy(), ref, rtol=1e-4, atol=1e-7)
        d = np.abs(b.out.cpu().numpy() - out["out"].detach().numpy()).sum(-1)
        assert d.max() <= 1e-4, f"step {step}: max per-vertex L1 {d.max():.3e}"
        assert np.abs(b.z.cpu().numpy() - out["z"].detach().numpy()).max() <= 1e-5
        hip_grads = {k: g.detach().cpu().clone() for k, g in eng.grads().items()}
        assert set(hip_grads) == set(grads)
        for name, g in hip_grads.items():
            close(g, grads[name], 1e-4, f"step {step} grad {name}")
        shadow_opt.step(shadow, hip_grads)
        sd = eng.state_dict()
        for name in weights:
            close(sd[name], shadow[name], 1e-6, f"step {step} adam {name}")
            assert (sd[name].cpu() - P[name].detach()).abs().max() <= 2e-4 * (step + 1) + 1e-6
