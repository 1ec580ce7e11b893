"""CPU tests of the general-shape SpiralConv host side: the new entry points
refuse bad arguments before any launch, ``cfsd_spiral_conv_has_shape`` agrees
with what the specialised entry points take, and the driver's configuration
check names the YAML key it refuses.  No kernel is launched here."""
import os

import pytest

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD_DATA, BWD_WEIGHT = ops.CONV_FWD, ops.CONV_BWD_DATA, ops.CONV_BWD_WEIGHT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def test_abi_minor_and_limits(lib):
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 19
    src = open(os.path.join(ROOT, "include", "cfsd.h")).read()
    assert f"#define CFSD_GEN_MAX_SEQ {ops.GEN_MAX_SEQ}\n" in src
    assert f"#define CFSD_GEN_MAX_CH {ops.GEN_MAX_CH}\n" in src
    for name, role in (("FWD", FWD), ("BWD_DATA", BWD_DATA), ("BWD_WEIGHT", BWD_WEIGHT),
                       ("BWD_FUSED", ops.CONV_BWD_FUSED)):
        assert f"#define CFSD_CONV_{name} {role}\n" in src


def _gen_rejections():
    """(entry point, defect, arguments, expected code), made-up pointers as in
    test_host_logic._conv_rejections: 64 is non-null and 16-B aligned; batch
    16, vsrc = rows = 40, spiral length 7, 8 -> 20 channels, an ample
    workspace unless the defect is its size."""
    P, WS, TINY = 64, 1 << 40, 64
    B, V, R = 16, 40, 40
    SMAX, CMAX = ops.GEN_MAX_SEQ, ops.GEN_MAX_CH

    def fwd(x=P, seq=7, cin=8, cout=20, act=0):
        return [x, P, P, P, P, B, V, R, seq, cin, cout, act, None]

    def bwd_data(w=P, seq=7, cin=8, cout=20):
        return [P, P, P, w, P, P, B, V, R, seq, cin, cout, None]

    def bwd_weight(dpre=P, db=P, ws_ptr=P, ws=WS, seq=7, cin=8, cout=20):
        return [P, P, dpre, P, db, ws_ptr, ws, B, V, R, seq, cin, cout, None]

    def dw_reduce(dw=P, ws=WS, seq=7, cin=8, cout=20):
        return [P, ws, dw, P, B, R, seq, cin, cout, None]

    return [
        ("gen_fwd", "null x", fwd(x=None), -1),
        ("gen_fwd", "seq 0", fwd(seq=0), -1),
        ("gen_fwd", "seq above the limit", fwd(seq=SMAX + 1), -1),
        ("gen_fwd", "cin above the limit", fwd(cin=CMAX + 1), -1),
        ("gen_fwd", "cout above the limit", fwd(cout=CMAX + 1), -1),
        ("gen_fwd", "act 7", fwd(act=7), -1),
        ("gen_bwd_data", "null w", bwd_data(w=None), -1),
        ("gen_bwd_data", "seq 0", bwd_data(seq=0), -1),
        ("gen_bwd_data", "seq above the limit", bwd_data(seq=SMAX + 1), -1),
        ("gen_bwd_data", "cin above the limit", bwd_data(cin=CMAX + 1), -1),
        ("gen_bwd_data", "cout above the limit", bwd_data(cout=CMAX + 1), -1),
        ("gen_bwd_weight", "null dpre", bwd_weight(dpre=None), -1),
        ("gen_bwd_weight", "null workspace", bwd_weight(ws_ptr=None), -1),
        ("gen_bwd_weight", "seq 0", bwd_weight(seq=0), -1),
        ("gen_bwd_weight", "seq above the limit", bwd_weight(seq=SMAX + 1), -1),
        ("gen_bwd_weight", "cin above the limit", bwd_weight(cin=CMAX + 1), -1),
        ("gen_bwd_weight", "cout above the limit", bwd_weight(cout=CMAX + 1), -1),
        ("gen_bwd_weight", "64-byte workspace", bwd_weight(ws=TINY), -2),
        ("gen_bwd_weight", "dw set, db null", bwd_weight(db=None), -1),
        ("gen_dw_reduce", "null dw", dw_reduce(dw=None), -1),
        ("gen_dw_reduce", "seq 0", dw_reduce(seq=0), -1),
        ("gen_dw_reduce", "cin above the limit", dw_reduce(cin=CMAX + 1), -1),
        ("gen_dw_reduce", "64-byte workspace", dw_reduce(ws=TINY), -2),
    ]


def test_general_entry_points_reject_before_launch(lib):
    import torch
    if torch.cuda.is_available():
        # a case that a defect lets through would launch on the made-up pointers
        pytest.skip("made-up pointers: only where no launch can reach a device")
    for entry, defect, args, want in _gen_rejections():
        rc = getattr(lib, "cfsd_spiral_conv_" + entry)(*args)
        msg = lib.cfsd_last_error_string()
        assert rc == want, (entry, defect, rc, msg)
        if "limit" in defect:
            assert b"limits" in msg, (entry, defect, msg)
        if defect == "dw set, db null":
            assert b"dw and db" in msg
        if want == -2:
            assert b"workspace" in msg


def test_general_workspace_query(lib):
    q = lib.cfsd_spiral_conv_gen_bwd_weight_workspace
    assert q(16, 40, 7, 8, 20) > 0 and q(1, 5, 1, 1, 1) > 0
    assert q(16, 40, 9, 32, 32) > 0  # the general family takes specialised shapes too
    for bad in ((0, 40, 7, 8, 20), (16, 0, 7, 8, 20), (16, 40, 0, 8, 20), (16, 40, ops.GEN_MAX_SEQ + 1, 8, 20),
                (16, 40, 7, ops.GEN_MAX_CH + 1, 20), (16, 40, 7, 8, ops.GEN_MAX_CH + 1)):
        assert q(*bad) == 0, bad
    # slabs of [cout * seq * cin + cout] floats
    assert q(16, 40, 7, 8, 20) % (4 * (20 * 7 * 8 + 20)) == 0


def test_has_shape_agrees_with_the_entry_points(lib):
    """Over the grid, a role is 1 exactly where the specialised entry point
    gets past its shape dispatch.  Forward and data gradient are probed with
    made-up pointers (no device: whatever is accepted could launch), the weight
    gradient through its workspace query."""
    import torch
    P, WS, B, V, R = 64, 1 << 40, 16, 40, 40
    probe = not torch.cuda.is_available()
    n_true = {FWD: 0, BWD_DATA: 0, BWD_WEIGHT: 0}
    for seq in (7, 9, 12):
        for cin in (3, 8, 16, 32, 48, 64):
            for cout in (3, 5, 16, 32, 64):
                has = {r: lib.cfsd_spiral_conv_has_shape(r, seq, cin, cout) for r in n_true}
                assert set(has.values()) <= {0, 1}
                for r in n_true:
                    n_true[r] += has[r]
                ws = lib.cfsd_spiral_conv_bwd_weight_workspace(B, R, seq, cin, cout)
                assert has[BWD_WEIGHT] == (1 if ws > 0 else 0), (seq, cin, cout, ws)
                assert ops.spiral_conv_has_shape(FWD, seq, cin, cout) == bool(has[FWD])
                if seq != 9:
                    assert not any(has.values()), (seq, cin, cout)
                if not probe:
                    continue
                # a shape WITHOUT an instance is refused with "unsupported" / "spiral length" before
                # any launch; one with an instance is only probed by has_shape (it would launch)
                if not has[FWD]:
                    rc = lib.cfsd_spiral_conv_fwd(P, P, P, P, P, P, WS, B, V, R, seq, cin, cout, 0, None)
                    msg = lib.cfsd_last_error_string()
                    assert rc == -1 and (b"unsupported" in msg or b"spiral length" in msg), (seq, cin, cout, msg)
                if not has[BWD_DATA]:
                    rc = lib.cfsd_spiral_conv_bwd_data(P, P, P, P, P, P, P, P, WS, B, V, R, seq, cin, cout, None)
                    msg = lib.cfsd_last_error_string()
                    assert rc == -1 and (b"unsupported" in msg or b"spiral length" in msg), (seq, cin, cout, msg)
                if not has[BWD_WEIGHT]:
                    rc = lib.cfsd_spiral_conv_bwd_weight(P, P, P, P, P, P, WS, B, V, R, seq, cin, cout, None)
                    assert rc == -1, (seq, cin, cout)
    # the lists themselves: 32/64 x 32/64, the xyz input (3 -> 16/32/64) and output (16/32/64 -> 3)
    assert n_true == {FWD: 4 + 3 + 3, BWD_DATA: 4 + 3, BWD_WEIGHT: 4 + 3 + 3}
    for r in n_true:
        assert lib.cfsd_spiral_conv_has_shape(r, 9, 32, 32) == 1
        assert lib.cfsd_spiral_conv_has_shape(r, 9, 0, 32) == 0
    assert lib.cfsd_spiral_conv_has_shape(4, 9, 32, 32) == 0 and lib.cfsd_spiral_conv_has_shape(-1, 9, 32, 32) == 0
    # the refusals test_host_logic pins stay refusals
    assert lib.cfsd_spiral_conv_bwd_weight_workspace(16, 17039, 9, 7, 5) == 0
    assert ops.spiral_conv_bwd_is_general(9, 3, 16) and not ops.spiral_conv_bwd_is_general(9, 3, 16, dx=False)
    assert ops.spiral_conv_bwd_is_general(7, 32, 32) and not ops.spiral_conv_bwd_is_general(9, 64, 32)


def test_fused_backward_keeps_its_shapes(lib):
    """``cfsd_spiral_conv_bwd`` has a fused launch of its own for the small-output layers
    32 / 64 -> 1, 2, 3, four of which (-> 1, 2) neither the data nor the weight gradient
    entry point has alone.  ``ops.spiral_conv_bwd`` and its workspace query stay with the
    library for all six, and for every shape its two entry points both take."""
    import torch
    P = 64
    fused = [(cin, cout) for cin in (32, 64) for cout in (1, 2, 3)]
    for cin in (1, 2, 3, 16, 32, 48, 64):
        for cout in (1, 2, 3, 4, 16, 32, 64):
            f = lib.cfsd_spiral_conv_has_shape(ops.CONV_BWD_FUSED, 9, cin, cout)
            assert f == int((cin, cout) in fused), (cin, cout)
            assert lib.cfsd_spiral_conv_has_shape(ops.CONV_BWD_FUSED, 7, cin, cout) == 0
            # without dx cfsd_spiral_conv_bwd takes its fused shapes and whatever _bwd_weight takes
            takes = bool(f) or bool(lib.cfsd_spiral_conv_has_shape(BWD_WEIGHT, 9, cin, cout))
            assert ops.spiral_conv_bwd_is_general(9, cin, cout, dx=False) == (not takes), (cin, cout)
            if not takes and not torch.cuda.is_available():  # made-up pointers: refused before any launch
                rc = lib.cfsd_spiral_conv_bwd(P, P, P, P, P, P, P, None, None, P, P, P, 1 << 40, 16, 40, 40, 9, cin,
                                              cout, None)
                assert rc == -1, (cin, cout)
    for cin, cout in fused:
        assert not ops.spiral_conv_bwd_is_general(9, cin, cout)
        assert ops.spiral_conv_vm_has_shape(9, cin, cout) and not ops.spiral_conv_vm_has_shape(7, cin, cout)
        assert ops.spiral_conv_bwd_workspace(16, 40, 40, 9, cin, cout) == \
            lib.cfsd_spiral_conv_bwd_workspace(16, 40, 40, 9, cin, cout) > 0
    # -> 1, 2: no instance of the separate entry points (their forward and dx alone are general)
    for cin, cout in ((32, 1), (32, 2), (64, 1), (64, 2)):
        assert not any(lib.cfsd_spiral_conv_has_shape(r, 9, cin, cout) for r in (FWD, BWD_DATA, BWD_WEIGHT))
    # the xyz input conv 1, 2, 3 -> 32 / 64 (no dx) stays with the library too
    for cin in (1, 2, 3):
        assert not ops.spiral_conv_bwd_is_general(9, cin, 32, dx=False) and ops.spiral_conv_vm_has_shape(9, cin, 64)
    assert not ops.spiral_conv_vm_has_shape(9, 48, 32) and ops.spiral_conv_vm_has_shape(9, 32, 64)


def test_ops_workspace_routing(lib):
    """ops sizes the weight-gradient workspace from the family that will run."""
    assert ops.spiral_conv_bwd_weight_workspace(16, 40, 9, 32, 32) == \
        lib.cfsd_spiral_conv_bwd_weight_workspace(16, 40, 9, 32, 32)
    assert ops.spiral_conv_bwd_weight_workspace(16, 40, 7, 8, 20) == \
        lib.cfsd_spiral_conv_gen_bwd_weight_workspace(16, 40, 7, 8, 20) > 0
    assert ops.spiral_conv_bwd_workspace(16, 40, 40, 12, 12, 40) == \
        lib.cfsd_spiral_conv_gen_bwd_weight_workspace(16, 40, 12, 12, 40)
    assert ops.spiral_conv_bwd_workspace(16, 40, 40, 9, 32, 3) == \
        lib.cfsd_spiral_conv_bwd_workspace(16, 40, 40, 9, 32, 3)


def _model(length, out_channels, **kw):
    return dict({"sampling": {"type": "basic", "sampling_factors": [4] * len(out_channels)},
                 "spirals": {"length": length, "dilation": [1] * len(length)}, "in_channels": 3,
                 "out_channels": out_channels, "latent_size": 22}, **kw)


def test_manager_config_check():
    from craniofacialsd_vae_amd import manager as M
    M.check_model_config(_model([7, 12], [8, 20]))
    M.check_model_config(_model([9, 9, 9, 9], [32, 32, 32, 64]))
    with pytest.raises(ValueError, match=r"model\.out_channels"):
        M.check_model_config(_model([7, 12], [6, 20]))
    with pytest.raises(ValueError, match=r"model\.spirals\.length"):
        M.check_model_config(_model([7, ops.GEN_MAX_SEQ + 1], [8, 20]))
    with pytest.raises(ValueError, match=r"model\.spirals\.length"):
        M.check_model_config(_model([7, 0], [8, 20]))
    with pytest.raises(ValueError, match=r"model\.out_channels"):
        M.check_model_config(_model([7, 12], [8, ops.GEN_MAX_CH + 4]))
    with pytest.raises(ValueError, match=r"model\.spirals\.length"):
        M.check_model_config(_model([7, 12, 9], [8, 20]))
    with pytest.raises(ValueError, match=r"model\.in_channels"):
        M.check_model_config(_model([7, 12], [8, 20], in_channels=0))
