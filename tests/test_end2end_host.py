"""``classifier.mlp_training_type: end2end`` on the host: the configuration
checks of ``classify.classifier_params`` (reference ``model_manager.py:97-104``)
and the new entry point's place in the C ABI.  No GPU needed."""
import ctypes

import pytest

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi  # noqa: E402
from craniofacialsd_vae_amd import classify as C  # noqa: E402

BASE = {"main_model_type": "mlp", "mlp_training_type": "end2end", "mlp_hidden_features": [32, 16], "mlp_lr": 1e-3,
        "mlp_epochs": 2, "mlp_loss_weight": 0.5}


def cfg(bs=4, **changes):
    section = dict(BASE, **changes)
    return {"classifier": {k: v for k, v in section.items() if v is not ...}, "optimization": {"batch_size": bs}}


def test_end2end_is_refused_unless_asked_for():
    """A caller that cannot train the classifier inside the step keeps being
    refused; one that can (ModelManager passes end2end=True) gets the section."""
    with pytest.raises(NotImplementedError, match="end2end"):
        C.classifier_params(cfg())
    with pytest.raises(NotImplementedError, match="end2end"):
        C.classifier_params(cfg(), end2end=False)
    assert C.classifier_params(cfg(), end2end=True) == BASE
    with pytest.raises(TypeError):  # keyword-only
        C.classifier_params(cfg(), True)
    # 'after' is untouched by the switch, and needs no loss weight
    after = dict(BASE, mlp_training_type="after")
    del after["mlp_loss_weight"]
    assert C.classifier_params({"classifier": after}, end2end=True) == after
    with pytest.raises(ValueError, match="mlp_training_type"):
        C.classifier_params(cfg(mlp_training_type="both"), end2end=True)


@pytest.mark.parametrize("weight", [..., None, float("nan"), float("inf"), -float("inf"), "much", True, [1.0]])
def test_loss_weight_must_be_a_finite_number(weight):
    with pytest.raises(ValueError, match="mlp_loss_weight"):
        C.classifier_params(cfg(mlp_loss_weight=weight), end2end=True)


def test_loss_weight_as_yaml_writes_it():
    """PyYAML reads ``1e-3`` as a string; weights are taken through float()."""
    assert C.classifier_params(cfg(mlp_loss_weight="1e-3"), end2end=True)["mlp_loss_weight"] == "1e-3"
    assert C.classifier_params(cfg(mlp_loss_weight=0), end2end=True)["mlp_loss_weight"] == 0


def test_batch_size_limit():
    assert C.classifier_params(cfg(bs=16), end2end=True) == BASE
    with pytest.raises(ValueError, match="batch_size"):
        C.classifier_params(cfg(bs=17), end2end=True)


def test_abi_has_the_head_step():
    lib = _abi.load()
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 18
    assert "cfsd_mlp_head_step" in _abi.SIGNATURES and hasattr(lib, "cfsd_mlp_head_step")
    # argument checks come before any launch: they answer without a GPU
    dims = (ctypes.c_int * 3)(75, 8, 3)
    args = [None, 75, 5, None, None, 1, None, None, None, None, None, None, None, 0, None, None, 225, 1.0]
    tail = [0, 1e-4, 0.9, 0.999, 1e-8, 0.0, None]
    assert lib.cfsd_mlp_head_step(*args, dims, 2, 17, *tail) != 0     # bs 17
    assert b"batch 17" in lib.cfsd_last_error_string()
    wide = (ctypes.c_int * 3)(75, 1025, 3)
    assert lib.cfsd_mlp_head_step(*args, wide, 2, 4, *tail) != 0      # width 1025
    assert lib.cfsd_mlp_head_step(*args, dims, 7, 4, *tail) != 0      # 7 layers
    assert lib.cfsd_mlp_head_step(*args, dims, 2, 4, *tail) != 0      # null pointers
    assert b"null pointer" in lib.cfsd_last_error_string()
