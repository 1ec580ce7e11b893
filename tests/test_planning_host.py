"""CPU tests of the surgical-planning host side: the refusals of the three
entry points of ``csrc/planning.hip`` before any HIP call, the validation of
``planning.procedures``, the pairs-table reader, the composed-metric formulas on
hand-made raw values, and the two new steps of ``evaluate.py``.  No kernel is
launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, evaluation, ops  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def _refused(lib, rc, word, code=-1):
    assert rc == code and word in lib.cfsd_last_error_string(), (rc, lib.cfsd_last_error_string())


def _floats(*values):
    return (ctypes.c_float * len(values))(*values)


def _windows(*rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def test_abi_version_and_constants(lib):
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 22
    for name in ("cfsd_plan_targets", "cfsd_plan_tables", "cfsd_pair_metrics"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert ops.PLAN_MAX_LEVELS == 8 and ops.PLAN_MAX_STEPS == 2 ** 20 and ops.PLAN_MAX_FIRST == 64
    assert ops.PLAN_MAX_WINDOWS >= 16 and len(ops.PAIR_RAW) == 6
    assert evaluation.PLAN_STEPS == 5000 and evaluation.PLAN_LEVELS == (3.0, 2.0, 1.0) and evaluation.PLAN_FIRST == 8


def test_plan_targets_validates_before_any_hip_call(lib):
    p, lv = ctypes.c_void_p(16), _floats(3.0, 2.0, 1.0)

    def call(z=p, mean=p, whiten=p, levels=lv, maha=p, index=p, targets=p, n=4, ld=75, col0=0, d=75, s=3, steps=5000):
        return lib.cfsd_plan_targets(z, mean, whiten, levels, maha, index, targets, n, ld, col0, d, s, steps, None)

    for name in ("z", "mean", "whiten", "levels", "maha", "index", "targets"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(d=0), b"d=0")
    _refused(lib, call(d=129, ld=200), b"d=129")
    _refused(lib, call(n=0), b"bad sizes")
    _refused(lib, call(col0=-1), b"bad sizes")
    _refused(lib, call(col0=70, d=6), b"bad sizes")               # a window past the row
    _refused(lib, call(s=0), b"levels")
    _refused(lib, call(s=9), b"9 levels")
    _refused(lib, call(steps=1), b"steps=1")
    _refused(lib, call(steps=2 ** 20 + 1), b"steps=")
    _refused(lib, call(n=2 ** 25, ld=128, d=128), b"2^31")
    _refused(lib, call(levels=_floats(1.0, 2.0, 3.0)), b"descending")  # ascending
    _refused(lib, call(levels=_floats(3.0, 3.0, 1.0)), b"descending")  # not strictly
    _refused(lib, call(levels=_floats(3.0, 2.0, 0.0)), b"positive")
    _refused(lib, call(levels=_floats(3.0, 2.0, -1.0)), b"positive")
    _refused(lib, call(levels=_floats(float("inf"), 2.0, 1.0)), b"finite")
    _refused(lib, call(levels=_floats(float("nan"), 2.0, 1.0)), b"positive")


def test_plan_tables_validates_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)

    def call(z=p, targets=p, mask=p, tables=p, dist=p, n=2, latent=75, s=3, procedures=11, n_first=8):
        return lib.cfsd_plan_tables(z, targets, mask, tables, dist, n, latent, s, procedures, n_first, None)

    for name in ("z", "targets", "mask", "tables", "dist"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(latent=0), b"latent=0")
    _refused(lib, call(latent=129), b"latent=129")
    _refused(lib, call(n=0), b"bad sizes")
    _refused(lib, call(procedures=-1), b"bad sizes")
    _refused(lib, call(s=0), b"levels")
    _refused(lib, call(s=9), b"9 levels")
    _refused(lib, call(n_first=0), b"n_first=0")
    _refused(lib, call(n_first=65), b"n_first=65")
    _refused(lib, call(n=2 ** 20, procedures=2 ** 11), b"2^31")


def test_pair_metrics_validates_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)
    good = _windows((0, 75, 0, 0), (70, 5, 75, 5625))

    def call(pre=p, post=p, windows=good, mean=p, whiten=p, raw=p, n=4, latent=75, w=2, mean_floats=80,
             whiten_floats=5650):
        return lib.cfsd_pair_metrics(pre, post, windows, mean, whiten, raw, n, latent, w, mean_floats, whiten_floats,
                                     None)

    for name in ("pre", "post", "windows", "mean", "whiten", "raw"):
        _refused(lib, call(**{name: None}), b"null")
    _refused(lib, call(n=0), b"bad sizes")
    _refused(lib, call(latent=0), b"bad sizes")
    _refused(lib, call(w=0), b"windows")
    _refused(lib, call(w=ops.PLAN_MAX_WINDOWS + 1), b"windows")
    _refused(lib, call(n=2 ** 27, w=2), b"2^31")
    _refused(lib, call(windows=_windows((0, 75, 0, 0), (71, 5, 75, 5625))), b"window 1")    # past the row
    _refused(lib, call(windows=_windows((0, 0, 0, 0), (70, 5, 75, 5625))), b"window 0")     # empty
    _refused(lib, call(windows=_windows((-1, 5, 0, 0), (70, 5, 75, 5625))), b"window 0")
    _refused(lib, call(latent=200, windows=_windows((0, 129, 0, 0), (70, 5, 75, 5625))), b"window 0")  # too wide
    _refused(lib, call(mean_floats=79), b"offsets")                                            # mean past its array
    _refused(lib, call(whiten_floats=5649), b"offsets")
    _refused(lib, call(windows=_windows((0, 75, -1, 0), (70, 5, 75, 5625))), b"offsets")


def test_ops_reject_host_tensors_and_bad_arguments():
    z, mean, whiten = torch.zeros(4, 20), torch.zeros(20), torch.eye(20)
    with pytest.raises(ValueError, match="device tensor"):
        ops.plan_targets(z, mean, whiten)
    with pytest.raises(ValueError, match="device tensor"):
        ops.plan_tables(z, torch.zeros(4, 4, 20))
    with pytest.raises(ValueError, match="device tensor"):
        ops.pair_metrics(z, z, [(0, 20, 0, 0)], mean, whiten.reshape(-1))
    for bad in ((1.0, 2.0), (2.0, 2.0), (1.0, 0.0), (), tuple(range(9, 0, -1)), (float("inf"),), (float("nan"),)):
        with pytest.raises(ValueError, match="levels"):
            ops._plan_levels(bad)
    assert ops._plan_levels((3, 2, 1)) == [3.0, 2.0, 1.0]


# ---------------------------------------------------------------- planning.procedures
REGIONS = {"#aa0000": [0, 5], "#00bb00": [5, 10], 7: [10, 15]}


def test_procedures_default_to_one_per_region():
    assert evaluation.planning_procedures({}, REGIONS) == {"#aa0000": ["#aa0000"], "#00bb00": ["#00bb00"], "7": [7]}
    assert evaluation.planning_procedures({"planning": None}, REGIONS).keys() == {"#aa0000", "#00bb00", "7"}
    assert evaluation.planning_procedures({"planning": {}}, REGIONS)["7"] == [7]


def test_procedures_are_validated_against_the_regions():
    cfg = {"planning": {"procedures": {"monobloc": ["#aa0000", "7"], "lefort": ["#00bb00"]}}}
    assert evaluation.planning_procedures(cfg, REGIONS) == {"monobloc": ["#aa0000", 7], "lefort": ["#00bb00"]}
    assert list(evaluation.planning_procedures(cfg, REGIONS)) == ["monobloc", "lefort"]  # the configuration's order
    for bad in ({}, [], "monobloc", {"a": []}, {"a": "#aa0000"}, {"a": ["#cc0000"]}, {"a": ["7", 7]}, {"a": None},
                {"all_attributes": ["7"]}, {"x/y": ["7"]}, {"": ["7"]}, {"..": ["7"]}):
        with pytest.raises(ValueError, match="planning.procedures"):
            evaluation.planning_procedures({"planning": {"procedures": bad}}, REGIONS)


# ---------------------------------------------------------------- the pairs table
HEADER = "PID,Pre name,Post name,Surgery regions,Procedure,Syndrome\n"


def test_read_pairs_table(tmp_path):
    path = tmp_path / "pairs.csv"
    path.write_text(HEADER + "007, a_pre.obj ,a_post.obj,monobloc,Monobloc,Apert\n12,c_pre.obj,c_post.obj,lefort,LF3,Crouzon\n")
    frame = evaluation.read_pairs_table(str(path))
    assert list(frame["PID"]) == ["007", "12"] and list(frame["Pre name"]) == ["a_pre.obj", "c_pre.obj"]
    assert list(frame["Surgery regions"]) == ["monobloc", "lefort"] and list(frame["Syndrome"]) == ["Apert", "Crouzon"]
    extra = tmp_path / "extra.csv"  # further columns are kept
    extra.write_text(HEADER.strip() + ",Age\n1,a,b,p,P,S,30\n")
    assert list(evaluation.read_pairs_table(str(extra))["Age"]) == ["30"]


@pytest.mark.parametrize("text,word", [
    ("PID,Pre name,Post name,Procedure,Syndrome\n1,a,b,P,S\n", "Surgery regions"),   # a column missing
    (HEADER, "no rows"),
    (HEADER + "1,a,,p,P,S\n", "empty"),
    (HEADER + "1,a,b,p,P,S\n1,c,d,p,P,S\n", "more than once")])
def test_read_pairs_table_refuses(tmp_path, text, word):
    path = tmp_path / "bad.csv"
    path.write_text(text)
    with pytest.raises(ValueError, match=word):
        evaluation.read_pairs_table(str(path))


# ---------------------------------------------------------------- the composed metrics
def test_composed_metrics_on_hand_made_values():
    """``test.py:996-1081`` by hand.  Rows: the whole latent, then regions r0, r1, r2."""
    raw = np.array([[6.0, 2.0, 9.0, 3.0, 0.5, 4.0],     # (6-2)/2 = 2, (9-3)/3 = 2, 4*0.5/2 = 1
                    [3.0, 1.0, 0.0, 0.0, 1.0, 2.0],     # (3-1)/1 = 2, 2*1/1 = 2
                    [1.0, 4.0, 0.0, 0.0, -0.5, 8.0],    # (1-4)/4 = -0.75, 8*-0.5/4 = -1
                    [5.0, 5.0, 0.0, 0.0, 0.25, 2.0]])   # 0, 0.1
    out = evaluation.compose_pair_metrics(raw, ["r0", "r1", "r2"], ["r0", "r1"])
    assert out["global_metric"] == 2.0 and out["global_metric_l2"] == 2.0 and out["global_metric_directional"] == 1.0
    assert out["region_metrics"] == {"r0": {"metric_distances": 2.0, "metric_with_angle": 2.0},
                                     "r1": {"metric_distances": -0.75, "metric_with_angle": -1.0}}
    assert out["procedure_metric"] == (2.0 - 0.75) / 2
    weighted = evaluation.compose_pair_metrics(raw, ["r0", "r1", "r2"], ["r0", "r1"], {"r0": 0.5, "r1": 1.0, "r2": 0.1})
    assert weighted["procedure_metric"] == (0.5 * 2.0 + 1.0 * -0.75) / 2
    assert weighted["region_metrics"] == out["region_metrics"] and weighted["global_metric"] == 2.0
    one = evaluation.compose_pair_metrics(raw, ["r0", "r1", "r2"], ["r2"])
    assert one["procedure_metric"] == 0.0 and one["region_metrics"]["r2"]["metric_with_angle"] == 0.1
    # a zero displacement: NaN in the directional metrics and nowhere else
    raw[:, 4] = np.nan
    raw[:, 5] = 0.0
    still = evaluation.compose_pair_metrics(raw, ["r0", "r1", "r2"], ["r0"])
    assert np.isnan(still["global_metric_directional"]) and np.isnan(still["region_metrics"]["r0"]["metric_with_angle"])
    assert still["global_metric"] == 2.0 and still["global_metric_l2"] == 2.0 and still["procedure_metric"] == 2.0
    with pytest.raises(ValueError):
        evaluation.compose_pair_metrics(raw[:3], ["r0", "r1", "r2"], ["r0"])
    with pytest.raises(ValueError):
        evaluation.compose_pair_metrics(raw, ["r0", "r1", "r2"], [])


# ---------------------------------------------------------------- the steps and the command line
def test_tester_has_the_plan_and_prepost_steps():
    assert "plan" in evaluation.Tester.STEPS and "prepost" in evaluation.Tester.STEPS
    assert evaluation.Tester.STEPS[:7] == ("traversals", "embeddings", "classifiers", "generation", "metrics",
                                           "interpolate", "tsne")
    for name in ("interpolate_syndrome_to_normal", "evaluate_pre_post_pair", "evaluate_all_pre_post_pairs",
                 "classify_and_project", "save_postop_colourmap", "plan_to_normal"):
        assert callable(getattr(evaluation.Tester, name))


@pytest.mark.parametrize("argv,word", [
    (["--only", "plan"], "--patient"),
    (["--only", "metrics,plan"], "--patient"),
    (["--only", "prepost"], "--pairs"),
    (["--only", "prepost", "--pairs", "pairs.csv"], "--pairs-root"),
    (["--only", "prepost", "--pairs-root", "."], "--pairs")])
def test_a_step_without_its_arguments_is_a_parser_error(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        evaluation.evaluate_main(["--id", "x"] + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
