"""CPU tests of the classifier stage's host side (``classify.py``, the
argument checks of ``csrc/classify.hip``): no kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import classify_cases as cases
import recipe

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi  # noqa: E402
from craniofacialsd_vae_amd import classify as C  # noqa: E402

NEW_SYMBOLS = ("cfsd_class_stats_workspace", "cfsd_class_stats", "cfsd_discriminant_scores", "cfsd_mlp_fwd",
               "cfsd_mlp_workspace", "cfsd_mlp_train_steps")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def _dims(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_and_version(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _abi.SIGNATURES, name
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 16


def test_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(256)
    err = lib.cfsd_last_error_string
    big = 1 << 30

    def stats(n=100, ld=75, col0=0, d=75, c=4, nbytes=big):
        return lib.cfsd_class_stats(p, p, p, p, p, p, nbytes, n, ld, col0, d, c, None)

    assert stats(ld=129, d=129) == EINVAL and b"d <= 128" in err()
    assert stats(c=65) == EINVAL and b"classes <= 64" in err()
    assert stats(col0=71, d=5) == EINVAL and b"bad sizes" in err()
    assert stats(n=0) == EINVAL
    need = lib.cfsd_class_stats_workspace(100, 75, 4)
    assert need == 4 * (4 * 75 * 75 + 4 * 75 + 4)  # one slice below 2048 rows
    assert lib.cfsd_class_stats_workspace(50000, 75, 4) == 16 * need
    assert lib.cfsd_class_stats_workspace(100, 129, 4) == 0 and lib.cfsd_class_stats_workspace(100, 75, 65) == 0
    assert stats(nbytes=need - 1) == EINVAL and b"workspace" in err()

    def scores(d=75, c=4, cw=4, ld=75):
        return lib.cfsd_discriminant_scores(p, p, p, p, p, p, p, 10, ld, 0, d, c, cw, None)

    assert scores(d=129, ld=129) == EINVAL and scores(c=65, cw=65) == EINVAL
    assert scores(cw=2) == EINVAL and b"whitening" in err()

    good = _dims(75, 512, 128, 64, 4)
    assert lib.cfsd_mlp_fwd(p, p, p, p, _dims(1, 2, 3, 4, 5, 6, 7, 8), 7, 5, None) == EINVAL and b"layers" in err()
    assert lib.cfsd_mlp_fwd(p, p, p, p, _dims(75, 1025, 4), 2, 5, None) == EINVAL and b"width" in err()
    assert lib.cfsd_mlp_fwd(p, p, p, p, good, 4, 0, None) == EINVAL
    assert lib.cfsd_mlp_fwd(None, p, p, p, good, 4, 5, None) == EINVAL and b"null" in err()

    ws = lib.cfsd_mlp_workspace(good, 4, 4)
    assert ws == 4 * 4 * ((75 + 512 + 128 + 64) + (512 + 128 + 64 + 4))
    assert lib.cfsd_mlp_workspace(good, 4, 17) == 0 and lib.cfsd_mlp_workspace(good, 7, 4) == 0

    def steps(dims=good, n_layers=4, bs=4, nbytes=big, n_rows=48, n_steps=12, train=1):
        return lib.cfsd_mlp_train_steps(p, p, p, p, p, p, p, p, p, nbytes, None, dims, n_layers, n_rows, 0, bs,
                                        n_steps, train, 1e-4, 0.9, 0.999, 1e-8, 0.0, None)

    assert steps(bs=17) == EINVAL and b"batch" in err()
    assert steps(dims=_dims(1, 2, 3, 4, 5, 6, 7, 8), n_layers=7) == EINVAL and b"layers" in err()
    assert steps(dims=_dims(75, 2000, 128, 64, 4)) == EINVAL and b"width" in err()
    assert steps(nbytes=ws - 1) == EINVAL and b"workspace" in err()
    assert steps(n_steps=13) == EINVAL and b"rows" in err()


def test_mlp_state_dict_keys_match_the_reference():
    """model.py:191-203: nn.Sequential of Linear + ReLU under ``model``."""
    mlp = C.MLPClassifier(75, [512, 128, 64], 4, device="cpu", seed=1)
    assert list(mlp.state_dict().keys()) == [f"model.{2 * i}.{k}" for i in range(4) for k in ("weight", "bias")]
    assert [tuple(v.shape) for v in mlp.state_dict().values()] == [(512, 75), (512,), (128, 512), (128,), (64, 128),
                                                                    (64,), (4, 64), (4,)]
    # parameters are views of the one flat buffer, in state_dict order
    assert torch.equal(torch.cat([v.reshape(-1) for v in mlp.state_dict().values()]), mlp.flat)
    assert mlp.model[2].weight.data_ptr() == mlp.flat[75 * 512 + 512:].data_ptr()
    # nn.Linear's initial range, reproducible from the seed
    assert float(mlp.model[0].weight.abs().max()) <= 1 / np.sqrt(75)
    assert float(mlp.model[6].bias.abs().max()) <= 1 / np.sqrt(64)
    assert torch.equal(C.MLPClassifier(75, [512, 128, 64], 4, device="cpu", seed=1).flat, mlp.flat)
    with pytest.raises(ValueError):  # there is no CPU path for the kernels
        mlp(torch.zeros(2, 75))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_finish_matches_sklearn(name):
    """finish_qda / finish_lda fed float64 statistics against the
    scikit-learn fixture: decision values (LDA: row-centred), log-probabilities
    and the 2-D transform within 1e-5 of the largest reference value."""
    sk = np.load(os.path.join(recipe.HERE, "classify_sklearn.npz"))
    case = cases.make_case(name)
    x, y = cases.valid_rows(case)
    n_cls = case["n_classes"]
    count = np.array([(y == c).sum() for c in range(n_cls)])
    mean = np.stack([x[y == c].mean(0) for c in range(n_cls)])
    scatter = np.stack([(x[y == c] - mean[c]).T @ (x[y == c] - mean[c]) for c in range(n_cls)])
    col0, d = case["cols"]
    xt = case["zt"][:, col0:col0 + d].astype(np.float64)

    def decision(f):
        return np.stack([-0.5 * (((xt - f["means"][c]) @ f["whiten"][c % len(f["whiten"])]) ** 2).sum(1)
                         + f["offset"][c] for c in range(n_cls)], 1)

    q = C.finish_qda(count, mean, scatter)
    ref = sk[f"{name}.qda_decision"]
    assert np.abs(decision(q) - ref).max() <= 1e-5 * np.abs(ref).max()
    np.testing.assert_allclose(q["priors"], sk[f"{name}.qda_priors"], rtol=1e-12)
    np.testing.assert_allclose(q["means"], sk[f"{name}.qda_means"], atol=1e-12)
    assert np.array_equal(np.argmax(decision(q), 1), sk[f"{name}.qda_pred"])

    f = C.finish_lda(count, mean, scatter)
    dec, ref = decision(f), sk[f"{name}.lda_decision"]
    dec, ref = dec - dec.mean(1, keepdims=True), ref - ref.mean(1, keepdims=True)
    assert np.abs(dec - ref).max() <= 1e-5 * np.abs(ref).max()
    logp = decision(f) - np.log(np.exp(decision(f) - decision(f).max(1, keepdims=True)).sum(1, keepdims=True)) \
        - decision(f).max(1, keepdims=True)
    assert np.abs(logp - sk[f"{name}.lda_log_proba"]).max() <= 1e-5 * np.abs(sk[f"{name}.lda_log_proba"]).max()
    tr, ref = (xt - f["xbar"]) @ f["projection"], sk[f"{name}.lda_transform"]
    sign = np.sign((tr * ref).sum(0))
    assert np.abs(tr * sign - ref).max() <= 1e-5 * np.abs(ref).max()


def test_finish_refuses_a_class_of_one_row():
    with pytest.raises(ValueError):
        C.finish_qda([5, 1], np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)))
    with pytest.raises(ValueError):
        C.finish_lda([5, 1], np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)))


def test_class_order_and_weights():
    """Sorted class letters ('b' already folded into 'n'); weights 1 / count
    normalised to sum 1 (data_loading.py:152-161, model_manager.py:548-555)."""
    from craniofacialsd_vae_amd.data import labels_of
    names = ["n_000.obj", "a_001.obj", "b_002.obj", "c_003.obj", "augmented/m_004_005.obj", "n_006.obj", "m_007.obj",
             "a_008.obj", "n_009.obj"]
    counts = C.count_labels([labels_of(n) for n in names])
    assert counts == {"n": 4, "a": 2, "c": 1, "m": 2}
    c2i, w = C.class_order_and_weights(counts)
    assert c2i == {"a": 0, "c": 1, "m": 2, "n": 3}
    inv = np.array([1 / 2, 1 / 1, 1 / 2, 1 / 4])
    np.testing.assert_allclose(w, inv / inv.sum(), rtol=1e-6)
    assert w.dtype == np.float32 and abs(float(w.sum()) - 1) < 1e-6
    with pytest.raises(ValueError):
        C.class_order_and_weights({})
    # a class of the data set without a training mesh keeps its place, with weight 0
    c2i, w = C.class_order_and_weights({"n": 4, "c": 1}, classes="acn")
    assert c2i == {"a": 0, "c": 1, "n": 2}
    np.testing.assert_allclose(w, [0.0, 0.8, 0.2], rtol=1e-6)
    with pytest.raises(ValueError):
        C.class_order_and_weights({"x": 3}, classes="acn")


def test_configuration_checks():
    base = {"main_model_type": "qda", "mlp_training_type": "after", "mlp_hidden_features": [32, 16], "mlp_lr": 1e-3,
            "mlp_epochs": 2}
    assert C.classifier_params({"model": {}}) is None  # no section: nothing is constructed
    assert C.classifier_params({"classifier": base}) == base
    with pytest.raises(ValueError, match="svm"):
        C.classifier_params({"classifier": dict(base, main_model_type="svm")})
    with pytest.raises(NotImplementedError, match="end2end"):
        C.classifier_params({"classifier": dict(base, mlp_training_type="end2end")})


def test_manager_without_classifier_section_constructs_nothing():
    """ClassifierStage._init_classifiers on a configuration without the
    section: no classifier attribute appears, and the stage's methods say so."""

    class Stub(C.ClassifierStage):
        pass

    s = Stub()
    s._init_classifiers({"model": {}, "data": {}, "optimization": {}})
    assert s._classifier_params is None
    assert not any(hasattr(s, a) for a in ("classifier_mlp", "lda", "qda", "region_ldas", "region_qdas"))
    with pytest.raises(RuntimeError, match="classifier"):
        s.classify_latent(torch.zeros(1, 75))
