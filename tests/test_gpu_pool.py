"""The Pool SpMM family of pool_swap.hip / spmm_sched.h on synthetic matrices, bit for bit against a
sequential fp32 fold (the GPU tests need an MI355X; the two ``test_fold_*`` tests prove the fold on the CPU).

Reference: ``fold`` -- a NumPy float32 loop over the COO entries in file order,
``y[:, r] = y[:, r] + x[:, c] * float32(v)``, product and sum rounded separately.  It uses neither the
kernels nor ``topology.py``.  ELU epilogue ``ref * where(ey > 0, 1, ey + 1)`` in fp32; bf16 inputs are
upcast exactly, bf16 outputs are ``ref.to(bfloat16)``.  Every GPU assertion is ``torch.equal`` on an
output buffer pre-filled with NaN, so an element no thread stored fails too.

Matrices (seeded, columns drawn with replacement so long rows repeat columns, COO shuffled so file order
is not row order; 53 columns unless noted):
  ragged       row lengths 0 3 1 2 4 5 7 8 9 15 16 17 24 25 33 64 97 0: the chunk edges 3/4/5, 8/9, 16/17
               of spmm_row_chunks<3|4|8> and spmm_fold_prefetch<8>, empty rows first and last
  ragged_long  the same lengths cycled to 150 rows (scheduled launches of 9+ workgroups, remainder mod 8)
  short        longest row exactly 16: ``row_schedule`` returns None
  lonely       5 rows, only row 3 (17 entries) is non-empty
  one          one row, one entry, 3 columns
  uni K m      m rows of exactly K entries
and the transposes of ragged, ragged_long, short and one (``csr_transpose_from_coo`` against the fold of
the swapped COO; empty rows wherever a column is unused).

Forms, each compared with the fold (hence equal to each other): plain CSR (``ops.spmm_x``, and
``ops.spmm`` where both operands are batch-major fp32), ``order=row_schedule(ptr)``, ``order=arange(m)``,
``sched=scheduled_csr(.., schedule)``, ``sched=scheduled_csr(.., arange(m))`` (the engine's ``upT_nat``
form) and ``uniform=K``.  A row with no entry reaches spmm_fold_prefetch / spmm_fold_prefetch8 through
the ``order=`` and ``sched=`` forms; in natural order with row 0 empty its extent starts at offset 0
(ragged, ragged_long, lonely, the transposes).

Which kernel runs (read from the dispatch code; a test cannot observe it):
  cfsd_spmm_uniform launches spmm_uniform_vm_k<3, 4> when x and y are both vertex-major, elu_y is null,
  k == 3, batch * (c / 4) % 64 == 0 and n * batch * c * 4 < 0x7ffff000; otherwise spmm_uniform_k<k, 4>.
  With rowq = batch * c / 4: (8, 32), (16, 16), (4, 64) give rowq 64, one wave per row; (16, 32) gives 128,
  two.  A wave runs 4 rows, a workgroup 4 waves: m = 1, 3 (< 4), 4, 5, 6, 7, 37, 150 cover every m % 4,
  a last workgroup with idle waves (37 rows: 10 waves in 3 workgroups) and 10 / 19 workgroups (150 rows,
  remainder 2 / 3 mod 8 in xcd_block_of).  The same operands with elu_y given run spmm_uniform_k.
  (A one-vertex tensor is contiguous in either layout and ``ops`` passes it as batch-major -- the same
  bytes -- so m = 1 runs spmm_uniform_k; m = 3 is the vertex-major kernel's m < 4.)
  cfsd_spmm_sched_csr uses V = 8 channels per thread for bf16 x with c % 8 == 0 (spmm_fold_prefetch8),
  else V = 4; groups = 8 when x is batch-major and batch % 8 == 0, else 1; bpg = batch / groups; the
  UNI (wave-uniform slot) kernel when (bpg * c / V) % 64 == 0.  In SPMM_CASES:
    UNI      vm x: (16, 16 f32) 64, (16, 32 bf16) 64, (8, 64 bf16) 64, (16, 32 f32) 128, (16, 64 bf16) 128;
             batch-major x: (4, 64 f32) one group 64, (64, 32 f32) and (64, 64 bf16) 8 groups of 8 meshes 64
    not UNI  vm x: (8, 32 bf16) 32, (16, 12 bf16) 48, (16, 100 f32) 400 (slots wider than a wave that
             waves straddle), (8, 12) 24; batch-major x: (16, 64 f32) 8 groups of 2 meshes 32,
             (16, 20 bf16) 10, and every batch 1 / 3 case
  spmm_csr_k / spmm_uniform_k split ``total = batch * m * c / 4`` chunks into 8 groups of
  ``(total + 7) / 8``: totals 1 (one, batch 1, c 4), 3, 162 (ragged, batch 3, c 12) and others that are
  no multiple of 8 leave ragged or empty groups.
"""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

import cfsd_loader
from oracle import cfsd_oracle as O

cfsd_loader.load()
from craniofacialsd_vae_amd import ops, topology  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
F, H = "f32", "bf16"
DT = {F: torch.float32, H: torch.bfloat16}
NCOL = 53
RAGGED = (0, 3, 1, 2, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 33, 64, 97, 0)
SHORT = (0, 16, 3, 1, 0, 4, 5, 8, 9, 2, 16, 7, 0)
LENS = {
    "ragged": (RAGGED, NCOL),
    "ragged_long": (tuple(RAGGED[i % len(RAGGED)] for i in range(150)), NCOL),
    "short": (SHORT, NCOL),
    "lonely": ((0, 0, 0, 17, 0), NCOL),
    "one": ((1,), 3),
}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _lens(mat):
    """(row lengths, columns) of a named matrix; ``("uni", K, m)`` is m rows of K entries."""
    if isinstance(mat, tuple):
        _, k, m = mat
        return (k,) * m, NCOL
    return LENS[mat]


@functools.lru_cache(maxsize=None)
def coo(mat, transposed=False):
    """(row, col, val, (m, n)) in a shuffled file order; ``transposed``: the same entries, rows and
    columns swapped (the transpose in the same file order)."""
    lens, n = _lens(mat)
    rs = np.random.RandomState(_seed(mat) % (1 << 31))
    row = np.repeat(np.arange(len(lens)), lens)
    col = rs.randint(0, n, row.size)
    val = rs.standard_normal(row.size).astype(np.float32)
    p = rs.permutation(row.size)
    row, col, val = row[p], col[p], val[p]
    return (col, row, val, (n, len(lens))) if transposed else (row, col, val, (len(lens), n))


def fold(x, entries):
    """The reference: x float32 [B, n, C] -> float32 [B, m, C], one entry at a time in file order."""
    row, col, val, (m, n) = entries
    assert x.dtype == np.float32 and x.shape[1] == n
    y = np.zeros((x.shape[0], m, x.shape[2]), np.float32)
    for r, c, v in zip(row, col, val):
        y[:, r] = y[:, r] + x[:, c] * np.float32(v)
    return y


# ------------------------------------------------------------------ the fold itself (CPU)
HOST_MATS = [("ragged", False), ("ragged", True), ("ragged_long", False), ("ragged_long", True),
             ("short", False), ("short", True), ("lonely", False), ("one", False), ("one", True),
             (("uni", 1, 7), False), (("uni", 2, 37), False), (("uni", 3, 150), False), (("uni", 4, 5), False)]
HOST_SHAPES = [(b, c) for c in (4, 12, 32, 100) for b in (1, 3, 16)]


def _host_x(mat, tr, b, c):
    n = coo(mat, tr)[3][1]
    return np.random.RandomState(_seed("x", mat, tr, b, c) % (1 << 31)).standard_normal((b, n, c)).astype(np.float32)


@pytest.mark.parametrize("mat,tr", HOST_MATS, ids=str)
def test_fold_equals_oracle_pool(mat, tr):
    """(a) the fold == oracle.cfsd_oracle.pool (index_select * value, sequential scatter_add) bit for bit."""
    for b, c in HOST_SHAPES:
        x = _host_x(mat, tr, b, c)
        ref = O.pool(torch.from_numpy(x), coo(mat, tr)).numpy()
        got = fold(x, coo(mat, tr))
        assert got.tobytes() == ref.tobytes(), f"{mat} T={tr} batch {b} c {c}"


@pytest.mark.parametrize("mat,tr", HOST_MATS, ids=str)
def test_fold_within_float64_bound(mat, tr):
    """(b) |fold - float64 sum| <= (L + 1) * 2^-24 * sum|x_e v_e| per output element, L the row
    length: L products and L adds, each within half an ulp."""
    row, col, val, (m, n) = coo(mat, tr)
    length = np.bincount(row, minlength=m).astype(np.float64)
    worst = 0.0
    for b, c in HOST_SHAPES:
        x = _host_x(mat, tr, b, c)
        s = np.zeros((b, m, c), np.float64)
        a = np.zeros((b, m, c), np.float64)
        for r, cc, v in zip(row, col, val):
            p = x[:, cc].astype(np.float64) * np.float64(v)
            s[:, r] += p
            a[:, r] += np.abs(p)
        err = np.abs(fold(x, coo(mat, tr)).astype(np.float64) - s)
        bound = (length[None, :, None] + 1) * 2.0 ** -24 * a
        assert np.all(err <= bound), f"{mat} T={tr} batch {b} c {c}: {np.max(err - bound):.3e} over"
        assert np.all(err[:, length == 0] == 0)
        nz = bound > 0
        if nz.any():
            worst = max(worst, float(np.max(err[nz] / bound[nz])))
    print(f"{mat} T={tr}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------ operands and forms
@functools.lru_cache(maxsize=None)
def device_matrix(mat, tr):
    """The matrix on the device in every form the wrappers take."""
    row, col, val, (m, n) = coo(mat, tr)
    build = topology.csr_transpose_from_coo if tr else topology.csr_from_coo
    # the transpose is built from the UNSWAPPED file (its first argument is the row of the original)
    ptr, ccol, cval = build(col, row, val, m) if tr else build(row, col, val, m)

    def dev(*arrays):
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)

    nat = np.arange(m, dtype=np.int32)
    schedule = topology.row_schedule(ptr)
    M = types.SimpleNamespace(m=m, n=n, ptr=ptr, csr=dev(ptr, ccol, cval), schedule=schedule)
    M.forms = {"csr": {}, "order_nat": dict(order=dev(nat)[0]),
               "nat": dict(sched=dev(*topology.scheduled_csr(ptr, ccol, cval, nat)))}
    if schedule is not None:
        M.forms["order"] = dict(order=dev(schedule)[0])
        M.forms["sched"] = dict(sched=dev(*topology.scheduled_csr(ptr, ccol, cval, schedule)))
    k = topology.uniform_rows(ptr)
    if k:
        M.forms["uniform"] = dict(uniform=k)
    return M


@functools.lru_cache(maxsize=None)
def operands(mat, tr, bsz, c, xdt):
    """(x in its storage type, the fold of x in fp32, an ELU output for the epilogue in fp32), on the
    host.  The ELU output holds, in every row, values > 0, exactly 0.0 (factor 1), just below 0 and
    -1.0 (factor 0)."""
    entries = coo(mat, tr)
    m, n = entries[3]
    g = torch.Generator().manual_seed(_seed("op", mat, tr, bsz, c, xdt))
    x = torch.randn(bsz, n, c, generator=g).to(DT[xdt])
    ref = torch.from_numpy(fold(x.float().numpy(), entries))
    ey = O.elu(torch.randn(bsz, m, c, generator=g))
    flat = ey.view(-1)
    for start, v in ((0, 0.0), (1, -1.0), (2, -1e-7), (3, 0.75)):
        flat[start::7] = v
    return x, ref, ey


def expected(ref, ey, ydt):
    if ey is not None:
        eyf = ey.float()
        ref = ref * torch.where(eyf > 0, torch.ones_like(eyf), eyf + 1.0)
    return ref.to(ydt)


def place(t, vm):
    t = t.to(DEV)
    return ops.to_vm(t) if vm else t


def nan_out(bsz, m, c, dtype, vm):
    y = ops.vm_empty(bsz, m, c, dtype=dtype, device=DEV) if vm else torch.empty(bsz, m, c, dtype=dtype, device=DEV)
    return y.fill_(float("nan"))


def same(got, exp, what):
    got = got.cpu()
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()  # NaN != anything: unwritten elements count
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {exp.numel()} elements differ, first at {at}: "
                             f"got {got[at].item()!r}, want {exp[at].item()!r}")


def run_forms(mat, tr, bsz, c, xdt, ydt, xvm, yvm, elu, only=None):
    """Every form the operands' layouts allow against the fold; returns the forms that ran."""
    M = device_matrix(mat, tr)
    x, ref, ey32 = operands(mat, tr, bsz, c, xdt)
    ey = ey32.to(DT[ydt]) if elu else None
    exp = expected(ref, ey, DT[ydt])
    xd, eyd = place(x, xvm), (place(ey, yvm) if elu else None)
    ran = []
    for name, kw in M.forms.items():
        if only is not None and name not in only:
            continue
        if name in ("order", "order_nat") and (xvm or yvm):
            continue  # batch-major only (test_refusals)
        what = f"{mat} T={tr} batch {bsz} c {c} {xdt}->{ydt} xvm {xvm} yvm {yvm} elu {elu} form {name}"
        out = nan_out(bsz, M.m, c, DT[ydt], yvm)
        assert ops.spmm_x(M.csr, xd, M.m, elu_y=eyd, out=out, **kw) is out
        same(out, exp, what)
        if xdt == F and ydt == F and not xvm and not yvm:
            same(ops.spmm(M.csr, xd, M.m, elu_y=eyd, **kw), exp, what + " (ops.spmm)")
            out = nan_out(bsz, M.m, c, DT[ydt], yvm)
            ops.spmm(M.csr, xd, M.m, elu_y=eyd, out=out, **kw)
            same(out, exp, what + " (ops.spmm, out=)")
        ran.append(name)
    return ran


# (matrix, transposed, batch, c, x type, y type, x vertex-major, y vertex-major, ELU epilogue)
U = "uni"
SPMM_CASES = [
    ("one", 0, 1, 4, F, F, 0, 0, 0),              # total = 1: seven empty XCD groups
    ("one", 0, 3, 4, F, H, 0, 1, 1),              # total = 3 < 8
    ("one", 1, 1, 8, H, F, 1, 0, 0),              # 3 rows, one column, two rows empty
    ("one", 1, 8, 4, F, F, 0, 0, 1),
    ("lonely", 0, 1, 4, F, F, 0, 0, 0),           # every row empty but one
    ("lonely", 0, 8, 12, H, H, 0, 0, 1),
    ("lonely", 0, 3, 8, H, F, 1, 1, 0),
    ("lonely", 0, 16, 32, F, H, 1, 1, 1),
    ("ragged", 0, 1, 4, F, F, 0, 0, 1),
    ("ragged", 0, 3, 12, F, F, 0, 0, 0),          # total = 162, no multiple of 8; c / 4 = 3
    ("ragged", 0, 8, 8, H, H, 0, 0, 1),           # 8-channel bf16 threads, 8 groups of one mesh
    ("ragged", 0, 16, 20, H, F, 0, 0, 0),         # 4-channel bf16 threads, 8 groups of two meshes
    ("ragged", 0, 3, 20, F, H, 1, 0, 1),
    ("ragged", 0, 16, 32, H, H, 1, 1, 1),         # V = 8, UNI (64)
    ("ragged", 0, 8, 32, H, F, 1, 1, 0),          # V = 8, not UNI (32)
    ("ragged", 0, 16, 16, F, F, 1, 1, 0),         # UNI (64)
    ("ragged", 0, 16, 12, H, H, 1, 0, 0),         # V = 4 bf16, not UNI (48)
    ("ragged", 0, 8, 12, F, F, 1, 1, 1),          # not UNI (24)
    ("ragged", 0, 16, 100, F, F, 1, 1, 1),        # not UNI (400): waves straddle slots
    ("ragged", 0, 3, 100, F, H, 0, 1, 0),
    ("ragged", 0, 4, 64, F, F, 0, 0, 1),          # UNI, batch-major x, one group
    ("ragged", 0, 64, 32, F, H, 0, 0, 0),         # UNI, batch-major x, 8 groups of 8 meshes
    ("ragged", 0, 16, 64, F, F, 0, 1, 0),         # 8 groups of 2 meshes, not UNI (32)
    ("ragged", 0, 8, 64, H, H, 1, 0, 1),          # V = 8, UNI (64), y batch-major
    ("ragged", 0, 64, 64, H, H, 0, 0, 1),         # V = 8, UNI, batch-major x, 8 groups of 8 meshes (64)
    ("ragged", 0, 1, 32, H, H, 0, 0, 0),
    ("ragged", 1, 3, 8, F, F, 0, 0, 0),
    ("ragged", 1, 8, 12, F, H, 1, 1, 1),
    ("ragged", 1, 16, 32, H, F, 0, 1, 0),
    ("ragged", 1, 1, 20, H, H, 1, 0, 1),
    ("ragged_long", 0, 16, 32, F, F, 1, 1, 0),    # scheduled: 75 workgroups, UNI (128)
    ("ragged_long", 0, 16, 64, H, H, 1, 1, 1),    # V = 8: 75 workgroups, UNI (128)
    ("ragged_long", 0, 3, 12, H, F, 1, 0, 0),     # 6 workgroups (< 8: no remap)
    ("ragged_long", 0, 8, 20, F, H, 0, 0, 1),     # 8 groups x 3 workgroups
    ("ragged_long", 0, 1, 100, F, F, 0, 0, 0),    # one group, 15 workgroups
    ("ragged_long", 0, 16, 4, F, F, 1, 1, 1),     # 10 workgroups
    ("ragged_long", 1, 16, 8, H, H, 1, 1, 0),
    ("ragged_long", 1, 3, 32, F, F, 0, 0, 1),
    ("short", 0, 3, 4, F, F, 0, 0, 1),
    ("short", 0, 8, 32, H, H, 1, 1, 0),
    ("short", 0, 16, 12, F, H, 0, 1, 1),
    ("short", 1, 1, 64, H, F, 1, 0, 0),
    ((U, 1, 1), 0, 1, 4, F, F, 0, 0, 0),          # uniform, total = 1
    ((U, 1, 37), 0, 3, 12, H, H, 1, 1, 1),
    ((U, 1, 150), 0, 16, 32, F, H, 0, 0, 0),      # 3 workgroups per group, the last one partial
    ((U, 1, 5), 0, 8, 100, H, F, 0, 1, 1),
    ((U, 2, 3), 0, 1, 8, H, H, 0, 0, 1),
    ((U, 2, 150), 0, 8, 20, F, F, 1, 0, 0),
    ((U, 2, 7), 0, 16, 64, F, H, 1, 1, 0),
    ((U, 2, 37), 0, 3, 4, H, F, 0, 1, 1),
    ((U, 3, 6), 0, 3, 12, F, F, 0, 0, 0),
    ((U, 3, 150), 0, 1, 100, H, H, 0, 0, 1),
    ((U, 3, 37), 0, 16, 20, F, H, 1, 0, 0),       # vertex-major x only: spmm_uniform_k
    ((U, 3, 4), 0, 8, 32, H, F, 0, 1, 0),
    ((U, 3, 150), 0, 3, 32, F, F, 1, 1, 0),       # both vertex-major, rowq = 24: spmm_uniform_k
    ((U, 4, 4), 0, 1, 4, F, F, 0, 0, 1),
    ((U, 4, 150), 0, 16, 32, H, H, 1, 1, 0),
    ((U, 4, 5), 0, 3, 20, F, H, 0, 1, 1),
    ((U, 4, 37), 0, 8, 64, H, F, 1, 0, 0),
    ((U, 4, 6), 0, 16, 12, F, F, 0, 0, 0),
]


def test_case_table_covers_the_issue():
    """The parameter table reaches every item it was built for (host check of the table itself)."""
    cs = SPMM_CASES
    assert {t[3] for t in cs} >= {4, 8, 12, 20, 32, 64, 100}
    assert {t[2] for t in cs} >= {1, 3, 8, 16}
    assert {(t[4], t[5]) for t in cs} == {(F, F), (H, H), (F, H), (H, F)}
    assert {(t[6], t[7]) for t in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {t[3] for t in cs if t[4] == H} >= {8, 12, 20, 32}
    assert {t[8] for t in cs} == {0, 1}
    totals = {t[2] * coo(t[0], bool(t[1]))[3][0] * t[3] // 4 for t in cs}
    assert 1 in totals and any(v % 8 for v in totals if v > 8) and any(1 < v < 8 for v in totals)

    def uni(t):  # cfsd_spmm_sched_csr's choice
        v = 8 if t[4] == H and t[3] % 8 == 0 else 4
        groups = 8 if not t[6] and t[2] % 8 == 0 else 1
        return v, groups, (t[2] // groups * (t[3] // v)) % 64 == 0
    assert {uni(t) for t in cs} >= {(v, g, u) for v in (4, 8) for g in (1, 8) for u in (False, True)}
    assert topology.row_schedule(topology.csr_from_coo(*coo("short")[:3], len(SHORT))[0]) is None
    assert topology.row_schedule(topology.csr_from_coo(*coo("ragged")[:3], len(RAGGED))[0]) is not None
    for k in (1, 2, 3, 4):
        assert {t[0][2] for t in cs if isinstance(t[0], tuple) and t[0][1] == k} - {1, 3, 4, 5, 6, 7, 37, 150} == set()


@gpu
@pytest.mark.parametrize("mat,tr,bsz,c,xdt,ydt,xvm,yvm,elu", SPMM_CASES, ids=str)
def test_spmm_forms(mat, tr, bsz, c, xdt, ydt, xvm, yvm, elu):
    ran = run_forms(mat, bool(tr), bsz, c, xdt, ydt, xvm, yvm, elu)
    want = {"csr", "nat"}
    if not (xvm or yvm):
        want.add("order_nat")
    if max(_lens(mat)[0]) > 16 and not tr:
        want.add("sched")
    if isinstance(mat, tuple):
        want.add("uniform")
    assert want <= set(ran), (want, ran)


UVM_M = (1, 3, 4, 5, 6, 7, 37, 150)


@gpu
@pytest.mark.parametrize("xdt,ydt", [(F, F), (H, H), (F, H), (H, F)])
@pytest.mark.parametrize("bsz,c", [(8, 32), (16, 16), (4, 64), (16, 32)])
def test_spmm_uniform_vm(bsz, c, xdt, ydt):
    """spmm_uniform_vm_k (uniform-3, both operands vertex-major, no elu_y), and spmm_uniform_k on the
    same operands (elu_y given), against the fold and the plain CSR kernel."""
    assert (bsz * c // 4) % 64 == 0
    for m in UVM_M:
        for elu in (0, 1):
            ran = run_forms((U, 3, m), False, bsz, c, xdt, ydt, 1, 1, elu, only=("csr", "uniform"))
            assert ran == ["csr", "uniform"]


@gpu
def test_refusals():
    """Bad operands raise before any launch: the output buffer keeps its NaN fill."""
    M = device_matrix("ragged", False)
    m, n = M.m, M.n
    x = torch.randn(2, n, 8).to(DEV)
    xh = x.bfloat16()
    bad = (ValueError, RuntimeError)  # host check, or CfsdError from the library's own

    def refused(fn, x_, out, **kw):
        before = None if out is None else out.clone()
        with pytest.raises(bad):
            fn(M.csr, x_, m, out=out, **kw)
        torch.cuda.synchronize()
        if out is not None:
            assert torch.equal(torch.isnan(out), torch.isnan(before)) and torch.isnan(out).all()

    forms = [M.forms[k] for k in ("csr", "order", "order_nat", "sched", "nat")]
    # c % 4 != 0, in every form and in the uniform one
    x6 = torch.randn(2, n, 6).to(DEV)
    for kw in forms:
        refused(ops.spmm_x, x6, nan_out(2, m, 6, torch.float32, 0), **kw)
        refused(ops.spmm, x6, nan_out(2, m, 6, torch.float32, 0), **kw)
    U3 = device_matrix((U, 3, 5), False)
    x6u = torch.randn(2, U3.n, 6).to(DEV)
    with pytest.raises(bad):
        ops.spmm_x(U3.csr, x6u, 5, out=nan_out(2, 5, 6, torch.float32, 0), uniform=3)
    # uniform = 5, and uniform = K over a matrix that does not hold m * K entries
    U5 = device_matrix((U, 5, 4), False)
    assert "uniform" not in U5.forms and topology.uniform_rows(U5.ptr) == 0
    xu = torch.randn(2, U5.n, 8).to(DEV)
    for fn in (ops.spmm_x, ops.spmm):
        out = nan_out(2, 4, 8, torch.float32, 0)
        with pytest.raises(bad):
            fn(U5.csr, xu, 4, out=out, uniform=5)
        with pytest.raises(bad):
            fn(U5.csr, xu, 4, out=out, uniform=4)   # 20 entries != 4 x 4
        with pytest.raises(bad):
            fn(M.csr, x, m, out=nan_out(2, m, 8, torch.float32, 0), uniform=3)  # ragged rows
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    # order= takes batch-major operands only
    for order in ("order", "order_nat"):
        refused(ops.spmm_x, ops.to_vm(x), nan_out(2, m, 8, torch.float32, 0), **M.forms[order])
        refused(ops.spmm_x, x, nan_out(2, m, 8, torch.float32, 1), **M.forms[order])
        refused(ops.spmm_x, ops.to_vm(xh), nan_out(2, m, 8, torch.bfloat16, 1), **M.forms[order])
        refused(ops.spmm, ops.to_vm(x), nan_out(2, m, 8, torch.float32, 0), **M.forms[order])
        refused(ops.spmm, x, nan_out(2, m, 8, torch.float32, 1), **M.forms[order])
    # out / elu_y of the wrong shape, type or layout
    ey = torch.zeros(2, m, 8, device=DEV)
    for kw in forms:
        for fn in (ops.spmm_x, ops.spmm):
            refused(fn, x, nan_out(2, m + 1, 8, torch.float32, 0), **kw)
            refused(fn, x, nan_out(3, m, 8, torch.float32, 0), **kw)
            refused(fn, x, nan_out(2, m, 4, torch.float32, 0), **kw)
            refused(fn, x, nan_out(2, m, 16, torch.float32, 0)[:, :, ::2], **kw)  # neither layout
            refused(fn, x, nan_out(2, 8, m, torch.float32, 0).transpose(1, 2), **kw)
            refused(fn, x, nan_out(2, m, 8, torch.float32, 0), elu_y=ey[:, :-1], **kw)
            refused(fn, x, nan_out(2, m, 8, torch.float32, 0), elu_y=ey[:1], **kw)
            refused(fn, x, nan_out(2, m, 8, torch.float32, 0), elu_y=ey.bfloat16(), **kw)
            refused(fn, x, nan_out(2, m, 8, torch.float32, 0), elu_y=ops.to_vm(ey), **kw)
            refused(fn, x, nan_out(2, m, 8, torch.float32, 0), elu_y=torch.zeros(2, m, 16, device=DEV)[:, :, ::2], **kw)
        refused(ops.spmm_x, x, nan_out(2, m, 8, torch.float32, 1), elu_y=ey, **kw)  # vm out, batch-major elu_y
        refused(ops.spmm_x, x, None, **kw)  # spmm_x allocates nothing
    refused(ops.spmm, xh, nan_out(2, m, 8, torch.float32, 0))  # ops.spmm is fp32 only
