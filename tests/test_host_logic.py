"""CPU tests of the host side: C-ABI exports, index-table builders, engine
parameter layout.  No kernel is launched here (no GPU in the build container)."""
import ctypes
import os
import re

import numpy as np
import pytest

import cfsd_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, topology  # noqa: E402


def header_functions():
    src = open(os.path.join(ROOT, "include", "cfsd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cfsd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def test_library_exports_every_header_symbol(lib):
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(_abi.SIGNATURES), set(names) ^ set(_abi.SIGNATURES)


def test_version_and_error_reporting(lib):
    assert lib.cfsd_version() >> 16 == 4  # 4.0: CFSD_VM vertex-major operands
    # argument validation happens before any HIP call: safe without a GPU
    rc = lib.cfsd_spiral_conv_fwd(None, None, None, None, None, None, 0, 1, 1, 1, 9, 32, 32, 0, None)
    assert rc == -1
    assert b"null" in lib.cfsd_last_error_string()
    rc = lib.cfsd_spiral_conv_fwd(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), None,
                                  ctypes.c_void_p(16), None, 0, 1, 10, 10, 7, 32, 32, 0, None)
    assert rc == -1 and b"spiral length" in lib.cfsd_last_error_string()
    assert lib.cfsd_spiral_conv_bwd_weight_workspace(16, 17039, 9, 32, 32) > 0
    assert lib.cfsd_spiral_conv_bwd_weight_workspace(16, 17039, 9, 7, 5) == 0


def _conv_rejections():
    """(entry point, defect, arguments, expected code).  Made-up pointers: 64 is
    non-null and 16-B aligned, 72 misaligned; batch 16, vsrc = rows = 40, seq 9,
    an ample workspace unless the defect is its size."""
    P, ODD, WS, TINY = 64, 72, 1 << 40, 64
    F32, BF16, VM = 0, 1, 0x10
    B, V, R, S = 16, 40, 40, 9

    def fwd(cin=32, cout=32, act=0, y=P):
        return [P, P, P, P, y, P, WS, B, V, R, S, cin, cout, act, None]

    def fwd_x(x_dt, y_dt, cin=32, cout=32, w_bf16=P):
        return [P, x_dt, P, P, w_bf16, P, P, y_dt, B, V, R, S, cin, cout, 0, None]

    def bwd_data(cin=32, cout=32, inv_head=P, seq=S):
        return [P, P, P, inv_head, P, P, P, P, WS, B, V, R, seq, cin, cout, None]

    def bwd_weight(cin=32, cout=32, db=P, ws=WS):
        return [P, P, P, P, db, P, ws, B, V, R, S, cin, cout, None]

    def bwd(db=P, ws=WS):
        return [P, P, P, P, P, P, P, P, P, P, db, P, ws, B, V, R, S, 32, 3, None]

    def bwd_x(dpre_dt=F32, cout=3):
        return [P, F32, P, P, dpre_dt, P, P, P, P, P, P, P, P, P, WS, B, V, R, S, 32, cout, None]

    def bwd_weight_x(x_dt, dpre_dt, ws=WS):
        return [P, x_dt, P, P, dpre_dt, P, P, P, ws, B, V, R, S, 32, 32, None]

    def bwd_rowsub(cin=32, flat_width=8, inv_flat=P, ws=WS):
        return [P, P, P, inv_flat, flat_width, P, P, P, P, P, P, ws, B, V, R, S, cin, 32, None]

    def bwd_data_rowsub(dx_dt=F32, ws=WS):
        return [P, P, 8, P, P, P, dx_dt, P, ws, B, V, R, S, 32, 32, None]

    def bwd_data_flat(dpre_dt, dx_dt):
        return [P, dpre_dt, P, 8, P, P, P, dx_dt, B, V, R, S, 32, 32, None]

    def bwd_out_flat(dt, cout=3):
        return [P, dt, P, P, dt, P, 8, P, P, P, P, P, P, WS, B, V, R, S, 32, cout, None]

    def fwd_in_swap(x_dt=F32, cin=3):
        return [P, P, P, P, 4, 4, 5, P, x_dt, P, P, P, P, F32, V, R, cin, 32, 0, None]

    return [
        ("fwd", "48 -> 32", fwd(cin=48), -1),
        ("fwd", "act 7", fwd(act=7), -1),
        ("fwd", "null y", fwd(y=None), -1),
        ("fwd_x", "dtype 2", fwd_x(2, F32), -1),
        ("fwd_x", "fp32 batch-major 32 -> 32", fwd_x(F32, F32), -1),
        ("fwd_x", "bf16 vm x, null w_bf16", fwd_x(BF16 | VM, BF16 | VM, w_bf16=None), -1),
        ("fwd_x", "fp32 vm x with bf16 y", fwd_x(F32 | VM, BF16 | VM), -1),
        ("fwd_x", "3 -> 16 with bf16 y", fwd_x(F32, BF16, cin=3, cout=16), -1),
        ("bwd_data", "inv_head at 72", bwd_data(inv_head=ODD), -1),
        ("bwd_data", "32 -> 5", bwd_data(cout=5), -1),
        ("bwd_data", "seq 7", bwd_data(seq=7), -1),
        ("bwd_weight", "dw set, db null", bwd_weight(db=None), -1),
        ("bwd_weight", "64-byte workspace", bwd_weight(ws=TINY), -2),
        ("bwd_weight", "7 -> 5", bwd_weight(cin=7, cout=5), -1),
        ("bwd", "32 -> 3, 64-byte workspace", bwd(ws=TINY), -2),
        ("bwd", "32 -> 3, dw without db", bwd(db=None), -1),
        ("bwd_x", "bf16 dpre", bwd_x(dpre_dt=BF16), -1),
        ("bwd_x", "32 -> 32", bwd_x(cout=32), -1),
        ("bwd_weight_x", "fp32 vm x with bf16 dpre", bwd_weight_x(F32 | VM, BF16 | VM), -1),
        ("bwd_weight_x", "bf16 32 -> 32, 64-byte workspace", bwd_weight_x(BF16, BF16, ws=TINY), -2),
        ("bwd_rowsub", "flat_width 6", bwd_rowsub(flat_width=6), -1),
        ("bwd_rowsub", "64 -> 32", bwd_rowsub(cin=64), -1),
        ("bwd_rowsub", "inv_flat at 72", bwd_rowsub(inv_flat=ODD), -1),
        ("bwd_rowsub", "64-byte workspace", bwd_rowsub(ws=TINY), -2),
        ("bwd_data_rowsub", "dx dtype 2", bwd_data_rowsub(dx_dt=2), -1),
        ("bwd_data_rowsub", "64-byte workspace", bwd_data_rowsub(ws=TINY), -2),
        ("bwd_data_flat", "batch-major operands", bwd_data_flat(F32, F32), -1),
        ("bwd_data_flat", "fp32 vm dx with bf16 dpre", bwd_data_flat(BF16 | VM, F32 | VM), -1),
        ("bwd_out_flat", "32 -> 32", bwd_out_flat(F32 | VM, cout=32), -1),
        ("bwd_out_flat", "batch-major operands", bwd_out_flat(F32), -1),
        ("fwd_in_swap", "32 -> 32", fwd_in_swap(cin=32), -1),
        ("fwd_in_swap", "bf16 x", fwd_in_swap(x_dt=BF16), -1),
    ]


def test_conv_entry_points_reject_before_launch(lib):
    """Every conv entry point validates its arguments before its first launch
    and keeps its return code: CFSD_EINVAL (-1) for a bad argument,
    CFSD_EWORKSPACE (-2) for a workspace that is too small."""
    import torch
    if torch.cuda.is_available():
        # a case that a defect lets through would launch on the made-up pointers
        pytest.skip("made-up pointers: only where no launch can reach a device")
    cases = _conv_rejections()
    assert len(cases) == 32
    for entry, defect, args, want in cases:
        rc = getattr(lib, "cfsd_spiral_conv_" + entry)(*args)
        msg = lib.cfsd_last_error_string()
        assert rc == want, (entry, defect, rc, msg)
        if defect == "dw set, db null":
            assert b"dw and db" in msg
        if entry == "bwd_rowsub" and want == -2:
            assert b"workspace" in msg


def test_bwd_weight_x_slabs_code(lib):
    """cfsd_spiral_conv_bwd_weight_x_slabs: the CFSD_DW_* code a deferred
    cfsd_spiral_conv_bwd_weight_x leaves, -1 where the entry point refuses the
    operands.  A pure function (no device call), so it runs here."""
    F32, BF16, VM = 0, 1, 0x10
    PLAIN, BF16_SLABS, VM32 = (_abi.CONSTANTS["CFSD_DW_" + k] for k in ("PLAIN", "BF16", "VM32"))
    table = [
        ((F32 | VM, F32 | VM, 16, 32, 32), VM32),        # vertex-major fp32 32 -> 32, 16-mesh batches
        ((F32 | VM, F32, 16, 32, 32), PLAIN),            # ... needs both operands vertex-major
        ((F32 | VM, F32 | VM, 4, 32, 32), PLAIN),        # ... and batch % 16 == 0
        ((F32 | VM, F32 | VM, 16, 32, 64), PLAIN),       # ... and 32 -> 32
        ((F32, F32, 16, 64, 64), PLAIN),
        ((BF16 | VM, BF16 | VM, 16, 32, 32), BF16_SLABS),  # bf16 x: the bf16 MFMA kernels, dpre bf16 or fp32
        ((BF16, F32, 4, 64, 32), BF16_SLABS),
        ((F32, BF16, 16, 3, 32), PLAIN),                 # the xyz input layer, dpre bf16 or fp32
        ((F32 | VM, F32, 16, 3, 64), PLAIN),
        ((F32 | VM, BF16 | VM, 16, 32, 32), -1),         # fp32 x needs fp32 dpre
        ((BF16, BF16, 16, 32, 3), -1),                   # no _x weight gradient for the output layer
        ((BF16, BF16, 16, 3, 32), -1),                   # the input layer's x is fp32
        ((2, F32, 16, 32, 32), -1),                      # not a storage type
        ((F32, F32 | 0x20, 16, 32, 32), -1),             # an unknown flag
        ((F32, F32, 0, 32, 32), -1),
    ]
    for args, want in table:
        assert lib.cfsd_spiral_conv_bwd_weight_x_slabs(*args) == want, args
    assert (PLAIN, BF16_SLABS, VM32) == (0, 2, 3)


def test_inverse_spiral_matches_bruteforce():
    rs = np.random.RandomState(0)
    idx = rs.randint(0, 50, size=(80, 9))
    ptr, rows, head = topology.inverse_spiral(idx, 50)
    assert head.shape == (50 * 9, topology.INV_HEAD)
    longest = 0
    for u in range(50):
        for s in range(9):
            k = u * 9 + s
            got = rows[ptr[k]:ptr[k + 1]].tolist()
            exp = [r for r in range(80) if idx[r, s] == u]
            assert got == exp
            longest = max(longest, len(exp))
            for j in range(topology.INV_HEAD):
                assert head[k, j] == (exp[j] if len(exp) > j else -1)
    assert longest > topology.INV_HEAD  # the overflow path is exercised


def test_inverse_flat_matches_bruteforce(topo_npz):
    """Flattened spiral positions p = r*9 + s per source vertex, ascending
    (the reference's index_add_ order), -1 padded to a multiple of 4."""
    rs = np.random.RandomState(1)
    idx = rs.randint(0, 60, size=(30, 9))
    flat, width = topology.inverse_flat(idx, 60)
    assert width % 4 == 0 and flat.shape == (60, width)
    for u in range(60):
        exp = [p for p in range(30 * 9) if idx.reshape(-1)[p] == u]
        assert flat[u].tolist() == exp + [-1] * (width - len(exp))
    # the craniofacial Enblock subsets (levels 1-3) fit in 8 entries
    T = topology.DeviceTopology.from_npz(topo_npz, device="cpu")
    for lv in (1, 2, 3):
        tab, w = T.enc_flat[lv]
        assert w == 8 and tuple(tab.shape) == (T.n_verts[lv], 8)
    assert topology.inverse_flat(np.zeros((20, 9), np.int64), 1) == (None, 0)


def test_csr_keeps_file_order_and_transpose():
    row = np.array([2, 0, 2, 1, 0, 2])
    col = np.array([5, 1, 0, 3, 4, 2])
    val = np.arange(6, dtype=np.float32)
    ptr, c, v = topology.csr_from_coo(row, col, val, 3)
    assert ptr.tolist() == [0, 2, 3, 6]
    assert c.tolist() == [1, 4, 3, 5, 0, 2] and v.tolist() == [1, 4, 3, 0, 2, 5]
    tp, tc, tv = topology.csr_transpose_from_coo(row, col, val, 6)
    assert tp.tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert tc.tolist() == [2, 0, 2, 1, 0, 2]


def test_selection_detection(topo_npz):
    for l in range(4):
        sel = topology.selection_rows(topo_npz[f"down_{l}_row"], topo_npz[f"down_{l}_col"],
                                      topo_npz[f"down_{l}_val"], int(topo_npz[f"down_{l}_shape"][0]))
        assert sel is not None and len(np.unique(sel)) == len(sel)
        up = topology.selection_rows(topo_npz[f"up_{l}_row"], topo_npz[f"up_{l}_col"],
                                     topo_npz[f"up_{l}_val"], int(topo_npz[f"up_{l}_shape"][0]))
        assert up is None


def test_device_topology_tables_on_cpu(topo_npz):
    T = topology.DeviceTopology.from_npz(topo_npz, device="cpu")
    assert T.n_verts == [17039, 4260, 1065, 267, 67]
    assert all(T.enc_select)
    assert T.n_regions == 15 and tuple(T.region_mask.shape) == (15, 17039)
    # row subset of level 0 == spiral rows of the kept vertices
    sel = topology.selection_rows(topo_npz["down_0_row"], topo_npz["down_0_col"],
                                  topo_npz["down_0_val"], 4260)
    np.testing.assert_array_equal(T.enc_rows[0].numpy(), topo_npz["spiral_0"][sel])
    # Laplacian rows sum to zero (random walk: 1 - sum 1/deg)
    ptr, col, val = (t.numpy() for t in T.lap_csr)
    sums = np.add.reduceat(val.astype(np.float64), ptr[:-1])
    assert np.abs(sums).max() < 1e-6


def test_engine_parameter_layout():
    from craniofacialsd_vae_amd.engine import ModelSpec
    import recipe
    spec = ModelSpec()
    specs = spec.param_specs(67, [9, 9, 9, 9])
    ref = recipe.param_shapes()
    assert sorted(specs) == sorted(ref)
    assert spec.reference_order(67, [9, 9, 9, 9]) == [k for k, _ in ref]
    names = [k for k, _ in specs]
    # stacked encoder Linears: logvar (en_layers.4) then mu (en_layers.5), adjacent
    i = names.index("en_layers.4.weight")
    assert names[i + 1] == "en_layers.5.weight"
    assert names[i + 2: i + 4] == ["en_layers.4.bias", "en_layers.5.bias"]
    assert sum(int(np.prod(s)) for _, s in specs) == 1081881


def test_checkpoint_format_round_trip(topo_npz, tmp_path):
    """f4 host side: save_weights / resume (model_manager.py:682-706) on an
    engine held in host memory (no kernel runs): reference file names and
    payload keys, bit-identical round trip, and the optimizer.pt payload is
    accepted by torch.optim.Adam over the reference parameter order."""
    import torch
    from craniofacialsd_vae_amd import engine as E
    topo = topology.DeviceTopology.from_npz(topo_npz, device="cpu")
    a = E.SDVAEEngine(topo, E.ModelSpec(), device="cpu")
    g = torch.Generator().manual_seed(0)
    a.params.exp_avg.normal_(generator=g)
    a.params.exp_avg_sq.uniform_(generator=g)
    a.params.step.fill_(7)
    assert a.save_weights(str(tmp_path), 4).endswith("model_00000005.pt")
    assert sorted(os.listdir(tmp_path)) == ["model_00000005.pt", "optimizer.pt"]
    b = E.SDVAEEngine(topo, E.ModelSpec(), device="cpu")
    assert b.resume(str(tmp_path)) == 5
    for buf in ("data", "exp_avg", "exp_avg_sq", "step"):
        assert torch.equal(getattr(a.params, buf), getattr(b.params, buf)), buf
    ck = torch.load(tmp_path / "model_00000005.pt", weights_only=True)["model"]
    assert list(ck) == list(a.state_dict())
    opt = torch.optim.Adam([v.clone().requires_grad_() for v in ck.values()], lr=1e-4)
    opt.load_state_dict(torch.load(tmp_path / "optimizer.pt", weights_only=True)["optimizer"])
    assert len(opt.state) == len(ck)
    st = opt.state_dict()["state"][3]
    assert float(st["step"]) == 7.0
    bad = a.optimizer_state_dict()
    bad["state"][0]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError):
        b.load_optimizer_state_dict(bad)


def test_epoch_permutation_is_a_permutation_per_epoch():
    """Oracle restatement of the device epoch shuffle (cfsd_step_begin): each
    epoch is a permutation of [0, n), epochs differ, drop_last batching."""
    from oracle import cfsd_oracle as O
    for n in (1, 2, 3, 7, 64, 250, 1000):
        p0, p1 = O.epoch_permutation(9, 0, n), O.epoch_permutation(9, 1, n)
        assert sorted(p0.tolist()) == list(range(n)) == sorted(p1.tolist())
        if n > 3:
            assert not np.array_equal(p0, p1)
    b = O.epoch_batches(9, 2, 10, 4, perm=np.arange(100, 110))
    assert b.shape == (2, 4) and len(np.unique(b)) == 8 and b.min() >= 100


def test_engine_requires_laplacian(topo_npz):
    from craniofacialsd_vae_amd import engine as E
    npz = {k: v for k, v in topo_npz.items() if not k.startswith("lap_")}
    topo = topology.DeviceTopology.from_npz(npz, device="cpu")
    with pytest.raises(ValueError, match="Laplacian"):
        E.SDVAEEngine(topo, E.ModelSpec(), device="cpu")


# ---------------------------------------------------------------- the ABI read from cfsd.h
_REFUSED = {
    "double parameter": ("int cfsd_a(const float* x, double scale);", "cfsd_a"),
    "struct by value": ("typedef struct { int n; } cfsd_s;\nint cfsd_b(cfsd_s s, int n);", "cfsd_b"),
    "function pointer": ("int cfsd_c(void (*done)(int), int n);", "cfsd_c"),
    "variadic": ("int cfsd_d(const char* fmt, ...);", "cfsd_d"),
    "long parameter": ("int cfsd_e(long n);", "cfsd_e"),
    "array parameter": ("int cfsd_f(int dims[4]);", "cfsd_f"),
    "pointer return": ("float* cfsd_g(int n);", "cfsd_g"),
    # the attribute splits the prototype: the pattern misses it, the occurrence count sees it
    "split prototype": ("int cfsd_ok(int n);\nint cfsd_h(int n)\n    __attribute__((warn_unused_result));", "cfsd_h"),
    "float define": ("#define CFSD_X 1.5\nint cfsd_ok(int n);", "CFSD_X"),
    "expression define": ("#define CFSD_Y (CFSD_Z + 1)\n", "CFSD_Y"),
    "pointer among several fields": ("typedef struct { float *a, b; } cfsd_t;", "cfsd_t"),
}


@pytest.mark.parametrize("defect", sorted(_REFUSED))
def test_header_parser_refuses_rather_than_guesses(defect):
    text, named = _REFUSED[defect]
    with pytest.raises(_abi.CfsdError, match=named):
        _abi.parse_header(text)


def test_header_parser_reads_the_forms_the_header_uses():
    sigs, structs, consts = _abi.parse_header("""
/* a comment naming cfsd_nothing(int) and #define CFSD_NOT 3 */
#ifndef CFSD_H
#define CFSD_H
#ifdef __cplusplus
extern "C" {
#endif
#define CFSD_N (-2)
#define CFSD_FLAG 0x10 /* trailing comment */
#define CFSD_TEN 10
#define CFSD_TYPE(dt) ((dt) & 0xf)
const char* cfsd_a(void);
typedef struct {
  const float* workspace;
  float* dw;
  int batch, rows, fused;
} cfsd_slabs;
size_t cfsd_b(const cfsd_slabs* items, uint16_t* shadow,
              size_t n, unsigned long long seed,
              float lr, const int32_t* step, int k, void* stream);
#ifdef __cplusplus
}
#endif
#endif
""")
    P, I, F, Z, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_ulonglong
    assert sigs == {"cfsd_a": (ctypes.c_char_p, []), "cfsd_b": (Z, [P, P, Z, U, F, P, I, P])}
    assert structs == {"cfsd_slabs": [("workspace", P), ("dw", P), ("batch", I), ("rows", I), ("fused", I)]}
    assert consts == {"CFSD_N": -2, "CFSD_FLAG": 16, "CFSD_TEN": 10}


def test_dw_slabs_layout():
    """cfsd_dw_slabs as the compiler lays it out: three pointers, six ints."""
    assert ctypes.sizeof(_abi.DwSlabs) == 48
    names = ["workspace", "dw", "db", "batch", "vsrc", "rows", "cin", "cout", "fused"]
    assert [n for n, _ in _abi.DwSlabs._fields_] == names
    assert [getattr(_abi.DwSlabs, n).offset for n in names] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    assert len(_abi.SIGNATURES) == len(header_functions())


_HEADER_CONSTANTS = {
    "ops": ["ACT_NONE", "ACT_ELU", "DT_F32", "DT_BF16", "VM", "CONV_FWD", "CONV_BWD_DATA", "CONV_BWD_WEIGHT",
            "CONV_BWD_FUSED", "GEN_MAX_SEQ", "GEN_MAX_CH", "DW_PLAIN", "DW_FUSED", "DW_BF16", "DW_VM32",
            "BN_SYNC_INTS", "BN_SYNC_ERR", "RM_MAX_REGIONS", "RM_THREADS", "NN_TILE", "PF_GROUP", "PF_CULL",
            "PF_PREPARED", "RN_GROUP", "RN_MAX_SIZE", "CLS_MAX_D", "CLS_MAX_CLASSES", "MLP_MAX_LAYERS",
            "MLP_MAX_WIDTH", "MLP_MAX_BS"],
    "topology": ["INV_HEAD"],
}


@pytest.mark.parametrize("module,name", [(m, n) for m, ns in _HEADER_CONSTANTS.items() for n in ns])
def test_python_constants_are_the_headers(module, name):
    """The value comes from the header's own text, read here with a pattern
    of this test's (not through the parser under test)."""
    import importlib
    src = open(os.path.join(ROOT, "include", "cfsd.h")).read()
    m = re.search(rf"^#define CFSD_{name} \(?(-?(?:0x[0-9a-fA-F]+|\d+))\)?[ \t]*(?:/\*.*)?$", src, re.M)
    assert m, f"cfsd.h has no integer #define CFSD_{name}"
    mod = importlib.import_module("craniofacialsd_vae_amd." + module)
    assert getattr(mod, name) == int(m.group(1), 0) == _abi.CONSTANTS["CFSD_" + name]


def test_limits_and_fused_codes_keep_their_values():
    """The limits and slab codes that got a name in cfsd.h are the numbers the kernels were built with."""
    want = {"CLS_MAX_D": 128, "CLS_MAX_CLASSES": 64, "MLP_MAX_LAYERS": 6, "MLP_MAX_WIDTH": 1024, "MLP_MAX_BS": 16,
            "BN_SYNC_INTS": 608, "DW_REDUCE_MAX": 16, "DW_PLAIN": 0, "DW_FUSED": 1, "DW_BF16": 2, "DW_VM32": 3}
    assert {k: _abi.CONSTANTS["CFSD_" + k] for k in want} == want


@pytest.mark.parametrize("header,named", [
    (None, "no_such_dir"),                                            # no header at that path
    ("int cfsd_version(void);\n", "cfsd_dw_slabs"),                   # a header without the struct
    ("typedef struct { struct { int a; } in; } cfsd_dw_slabs;\n", "cfsd_dw_slabs"),  # a nested brace
])
def test_unreadable_header_is_a_cfsd_error(tmp_path, monkeypatch, header, named):
    """Importing the binding over a header it cannot use raises CfsdError naming the path or the struct."""
    import importlib.util
    path = tmp_path / "no_such_dir" / "cfsd.h" if header is None else tmp_path / "cfsd.h"
    if header is not None:
        path.write_text(header)
    monkeypatch.setenv("CFSD_HEADER_PATH", str(path))
    spec = importlib.util.spec_from_file_location("abi_probe", _abi.__file__)
    with pytest.raises(RuntimeError, match=named) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "CfsdError"


# ------------------------------------------------------------------ SpMM schedule builders
def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def test_row_schedule():
    lens = np.array([0, 3, 17, 1, 3, 0, 17, 40, 3, 1])
    order = topology.row_schedule(_ptr(lens))
    assert order.dtype == np.int32
    assert sorted(order.tolist()) == list(range(len(lens)))          # a permutation of the rows
    assert np.all(np.diff(lens[order]) <= 0)                         # lengths non-increasing
    assert order.tolist() == [7, 2, 6, 1, 4, 8, 3, 9, 0, 5]           # stable among equal lengths
    assert topology.row_schedule(_ptr([3, 16, 0, 16])) is None       # longest row exactly 16
    assert topology.row_schedule(_ptr([3, 17, 0, 16])).tolist() == [1, 3, 0, 2]
    assert topology.row_schedule(_ptr([])) is None                   # no rows
    assert topology.row_schedule(_ptr([0, 0])) is None
    assert topology.row_schedule(_ptr([2, 3]), min_max_len=2).tolist() == [1, 0]


def test_scheduled_csr():
    rs = np.random.RandomState(7)
    lens = np.array([0, 3, 17, 1, 0, 0, 5, 17, 2, 0])
    m, n, nnz = len(lens), 11, int(lens.sum())
    ptr, col, val = _ptr(lens), rs.randint(0, n, nnz).astype(np.int32), rs.standard_normal(nnz).astype(np.float32)
    order = topology.row_schedule(ptr)
    for visit in (order, np.arange(m), rs.permutation(m)):
        ptr_s, col_s, val_s, rows_s = topology.scheduled_csr(ptr, col, val, visit)
        assert (ptr_s.dtype, col_s.dtype, val_s.dtype, rows_s.dtype) == (np.int32, np.int32, np.float32, np.int32)
        assert rows_s.tolist() == list(visit)
        assert ptr_s.tolist() == [0] + np.cumsum(lens[visit]).tolist()  # cumulative visited lengths
        for i, r in enumerate(visit):                                 # each slot: that row's entries, in order
            assert col_s[ptr_s[i]:ptr_s[i + 1]].tolist() == col[ptr[r]:ptr[r + 1]].tolist()
            assert val_s[ptr_s[i]:ptr_s[i + 1]].tobytes() == val[ptr[r]:ptr[r + 1]].tobytes()
            if lens[r] == 0:
                assert ptr_s[i] == ptr_s[i + 1]                       # an empty row is an empty slot
        # scattering the slot results back by rows_s reproduces the plain CSR product
        x = rs.standard_normal((n, 4)).astype(np.float32)
        plain = np.stack([sum((x[col[e]] * val[e] for e in range(ptr[r], ptr[r + 1])), np.zeros(4, np.float32))
                          for r in range(m)])
        back = np.full((m, 4), np.nan, np.float32)
        for i in range(m):
            back[rows_s[i]] = sum((x[col_s[e]] * val_s[e] for e in range(ptr_s[i], ptr_s[i + 1])),
                                  np.zeros(4, np.float32))
        assert back.tobytes() == plain.tobytes()
    nat = topology.scheduled_csr(ptr, col, val, np.arange(m))      # natural order: the input CSR itself
    assert nat[0].tolist() == ptr.tolist() and nat[1].tolist() == col.tolist()
    assert nat[2].tobytes() == val.tobytes() and nat[3].tolist() == list(range(m))
    empty = topology.scheduled_csr(_ptr([0, 0]), col[:0], val[:0], [1, 0])
    assert empty[0].tolist() == [0, 0, 0] and empty[1].size == 0 and empty[2].size == 0
    none = topology.scheduled_csr(_ptr([]), col[:0], val[:0], [])
    assert none[0].tolist() == [0] and none[1].size == 0 and none[3].size == 0


def test_uniform_rows():
    for k in (1, 2, 3, 4):
        assert topology.uniform_rows(_ptr([k] * 6)) == k
        assert topology.uniform_rows(_ptr([k])) == k
    assert topology.uniform_rows(_ptr([0] * 6)) == 0               # k = 0
    assert topology.uniform_rows(_ptr([5] * 6)) == 0               # k = 5 > max_k
    assert topology.uniform_rows(_ptr([5] * 6), max_k=5) == 5
    assert topology.uniform_rows(_ptr([3, 3, 2, 3])) == 0          # mixed lengths
    assert topology.uniform_rows(_ptr([2, 3, 3, 3])) == 0
    assert topology.uniform_rows(_ptr([3, 3, 3, 4])) == 0
    assert topology.uniform_rows(_ptr([])) == 0                    # no rows
