"""Exact-value inputs and the fp64 restatement of one SpiralConv, for the
vertex-major and bf16 kernel tests.

TEST INFRASTRUCTURE, next to ``spiral_tables.py``; imports without loading the
library, so ``tests/test_exact_values_host.py`` runs everything here on the CPU.

A rounding bound is intrinsically weak for bf16: the inverse-table dx kernels
round the per-slot list sum ``A_s[u, o]`` to bf16 before the MFMA, and on a hub
vertex ``2^-8 * sum|terms|`` is larger than a whole lost list entry.  So the
kernel tests also run on inputs for which EVERY intermediate is exactly
representable and no result depends on the summation order:

  * x, w, b, dpre from {-1, -1/2, 0, 1/2, 1} (dpre from {-1, 0, 1} where the
    inverse-table bf16 kernels are under test), elu_y from
    {-1, -1/2, 0, 1/2, 1, 2}: all exact in bf16; ELU' = y + 1 or 1 is one of
    {0, 1/2, 1}.
  * every product is a multiple of 1/4 (1/8 after ELU'), so a partial sum of
    magnitude below 2^22 (2^21) is exact in fp32 in any order, and so is the
    MFMA accumulation whatever its internal order.

``assert_exact`` checks the two conditions this rests on from the restatement's
own ``*_abs`` tensors (sum of |terms| bounds every partial sum of every order).
"""
import numpy as np
import torch

DYADIC = (-1.0, -0.5, 0.0, 0.5, 1.0)
SIGNS = (-1.0, 0.0, 1.0)          # dpre of the inverse-table bf16 dx kernels
SPARSE_SIGNS = (-1.0, 0.0, 0.0, 0.0, 1.0)
ELU_OUT = (-1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
EXACT_LIMIT = 2.0 ** 24


def draw(g, shape, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def exact_inputs(g, batch, vsrc, rows, seq, cin, cout, dpre_values=DYADIC):
    """x, w, b, dpre, elu_y (fp32 tensors, in this draw order) from the dyadic sets."""
    return {"x": draw(g, (batch, vsrc, cin), DYADIC), "w": draw(g, (cout, seq * cin), DYADIC),
            "b": draw(g, (cout,), DYADIC), "dpre": draw(g, (batch, rows, cout), dpre_values),
            "elu_y": draw(g, (batch, vsrc, cin), ELU_OUT)}


ALL_PARTS = ("fwd", "dx", "dw")


def restate(idx, x, w, b, dpre, chunk=None, parts=ALL_PARTS):
    """fp64 restatement of forward, dx, dW, db and the sums of |terms| of each
    (index_select + matmul; dx by index_add_; dW by dY^T G), ``chunk`` rows at a
    time.  Tensors in, dict of fp64 tensors out.  ``parts``: which of "fwd"
    (pre), "dx", "dw" to compute (db always)."""
    batch, vsrc, cin = x.shape
    rows, seq = idx.shape
    cout = w.shape[0]
    x, w, b, dp = x.double(), w.double(), b.double(), dpre.double()
    chunk = rows if chunk is None else chunk
    pre, pre_abs = [], []
    r = {}
    if "dx" in parts:
        r["dx"] = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
        r["dx_abs"] = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
    if "dw" in parts:
        r["dw"] = torch.zeros(cout, seq * cin, dtype=torch.float64)
        r["dw_abs"] = torch.zeros(cout, seq * cin, dtype=torch.float64)
    for r0 in range(0, rows, chunk):
        r1 = min(r0 + chunk, rows)
        flat = idx[r0:r1].reshape(-1)
        if "fwd" in parts or "dw" in parts:
            G = x[:, flat].reshape(batch, r1 - r0, seq * cin)
        if "fwd" in parts:
            pre.append(G @ w.T + b)
            pre_abs.append(G.abs() @ w.abs().T + b.abs())
        dpc = dp[:, r0:r1]
        if "dx" in parts:
            dG = (dpc @ w).reshape(batch, (r1 - r0) * seq, cin)
            dG_abs = (dpc.abs() @ w.abs()).reshape(batch, (r1 - r0) * seq, cin)
            r["dx"].index_add_(1, flat, dG)
            r["dx_abs"].index_add_(1, flat, dG_abs)
        if "dw" in parts:
            G2, dp2 = G.reshape(batch * (r1 - r0), -1), dpc.reshape(batch * (r1 - r0), cout)
            r["dw"] += dp2.T @ G2
            r["dw_abs"] += dp2.abs().T @ G2.abs()
    if "fwd" in parts:
        r["pre"] = pre[0] if len(pre) == 1 else torch.cat(pre, 1)
        r["pre_abs"] = pre_abs[0] if len(pre_abs) == 1 else torch.cat(pre_abs, 1)
    dp2 = dp.reshape(batch * rows, cout)
    r["db"], r["db_abs"] = dp2.sum(0), dp2.abs().sum(0)
    return r


def restate_dx(idx, w, dpre, vsrc, chunk=None):
    """dx and its sum of |terms| alone (``restate``'s arithmetic), for a second dpre of a case."""
    batch, rows, cout = dpre.shape
    seq = idx.shape[1]
    cin = w.shape[1] // seq
    w, dp = w.double(), dpre.double()
    chunk = rows if chunk is None else chunk
    dx = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
    dx_abs = torch.zeros(batch, vsrc, cin, dtype=torch.float64)
    for r0 in range(0, rows, chunk):
        r1 = min(r0 + chunk, rows)
        flat = idx[r0:r1].reshape(-1)
        dpc = dp[:, r0:r1]
        dx.index_add_(1, flat, (dpc @ w).reshape(batch, (r1 - r0) * seq, cin))
        dx_abs.index_add_(1, flat, (dpc.abs() @ w.abs()).reshape(batch, (r1 - r0) * seq, cin))
    return dx, dx_abs


def slot_sums_max(idx, dpre, vsrc, check_bf16=True):
    """max |A_s[u, o]| over the per-slot list sums A_s[u, o] = sum of dpre[r, o] over
    the rows r with idx[r, s] == u (what conv_dx_b16 / conv_dx_vm16 round to bf16);
    with ``check_bf16`` asserts that every one of them round-trips through bf16."""
    batch, rows, cout = dpre.shape
    dp, worst = dpre.double(), 0.0
    for s in range(idx.shape[1]):
        A = torch.zeros(batch, vsrc, cout, dtype=torch.float64).index_add_(1, idx[:, s], dp)
        if check_bf16:
            assert torch.equal(A.to(torch.bfloat16).double(), A), f"slot {s}: a list sum is not exact in bf16"
        worst = max(worst, float(A.abs().max()))
    return worst


def assert_exact(ref, inverse_bf16=None):
    """The conditions of the exact mode, from the restatement ``ref`` (module
    docstring): |sum| * granularity denominator < 2^24 for every product.
    ``inverse_bf16``: (idx, dpre, vsrc) when an inverse-table bf16 dx kernel runs
    on the case -- its list sums must be exact in bf16.  Returns the margins."""
    scale = {"pre_abs": ("fwd", 4), "dx_abs": ("dx*elu'", 8), "dw_abs": ("dw", 4), "db_abs": ("db", 2)}
    out = {name: k * float(ref[key].max()) for key, (name, k) in scale.items() if key in ref}
    for k, v in out.items():
        assert v < EXACT_LIMIT, (k, v)
    if inverse_bf16 is not None:
        out["A"] = slot_sums_max(*inverse_bf16)
    return out


def seed_of(batch, vsrc, rows, cin, cout):
    return (batch * 7 + vsrc) * 131 + rows * 17 + cin * 3 + cout


# The exact cases of the GPU tests that the host test builds as well: (batch, vsrc, rows, table,
# cin, cout, dpre values, inverse-table bf16 dx runs on it).  The hub cases are the ones whose sums
# come nearest the limits (longest list rows // 2 / 3 on a hub key).
HOST_CASES = [
    (16, 4097, 4097, "hubs", 32, 32, SIGNS, True),
    (16, 8193, 8193, "hubs", 32, 64, DYADIC, False),
    (48, 1367, 1367, "hubs", 32, 32, SIGNS, True),
    (16, 4097, 4097, "head_edge", 32, 64, SIGNS, True),
    (3, 2731, 2731, "hubs", 64, 64, SIGNS, True),
    (16, 911, 2733, "hubs", 64, 32, SIGNS, True),
    (16, 2731, 683, "random", 32, 32, SIGNS, True),
    (1, 37, 37, "head_edge", 64, 64, SIGNS, True),
]


def as_index(table):
    return torch.as_tensor(np.asarray(table), dtype=torch.int64)
