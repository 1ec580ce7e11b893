"""CPU tests of the t-SNE host side: the float64 restatement (tsne_oracle.py)
pinned on what scikit-learn 1.7.2's own functions gave
(tests/golden/make_tsne.py -> tsne_sklearn.npz), the symmetrisation of ``ops``
on CPU tensors, the refusals of every new entry point before any HIP call, and
the host behaviour around them.  No kernel is launched, no scikit-learn is
imported."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import cfsd_loader

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, evaluation, ops, tsne  # noqa: E402

import tsne_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_sklearn.npz")
PERPLEXITY = 30.0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def oracle_p(gold):
    p_cond, beta = O.perplexity_search(gold["nn_d2"], PERPLEXITY)
    return p_cond, O.symmetrize(gold["nn_idx"], p_cond)


# Restatement against scikit-learn: each bound is four times the gap measured
# when the goldens were made (stored beside them; DESIGN section 14 quotes them:
# P 3.1e-16 of max P, gradient 1.1e-6 of max |grad|, KL 2.4e-6 relative -- the
# last two are the fp32 of _barnes_hut_tsne, the restatement is float64).
def test_oracle_affinities_match_sklearn(gold, oracle_p):
    p_cond, dense = oracle_p
    row_ptr, col, val = O.to_csr(dense)
    assert np.array_equal(row_ptr, gold["p_indptr"]) and np.array_equal(col, gold["p_indices"])
    gap = np.abs(val - gold["p_data"]).max() / gold["p_data"].max()
    print(f"P: restatement vs scikit-learn {gap:.3e} of max P (recorded {gold['gap_p']:.3e})")
    assert gap <= 4 * gold["gap_p"]
    assert np.abs(p_cond.sum(1) - 1).max() < 1e-12
    assert np.abs(O.entropy(p_cond) - np.log(PERPLEXITY)).max() <= 1e-5 + 1e-12


@pytest.mark.parametrize("name", ["small", "large"])
def test_oracle_gradient_and_kl_match_sklearn(gold, name):
    dense = O.from_csr(gold["p_indptr"], gold["p_indices"], gold["p_data"])
    kl, grad = O.kl_and_grad(dense, gold[f"y_{name}"])
    gap_g = np.abs(grad - gold[f"grad_{name}"]).max() / np.abs(grad).max()
    gap_k = abs(kl - gold[f"kl_{name}"]) / abs(kl)
    print(f"{name}: gradient {gap_g:.3e} of max |grad| (recorded {gold['gap_grad']:.3e}), "
          f"KL {gap_k:.3e} relative (recorded {gold['gap_kl']:.3e})")
    assert gap_g <= 4 * gold["gap_grad"]
    assert gap_k <= 4 * gold["gap_kl"]


def test_oracle_update_rule_is_gradient_descents():
    """The four sign / gain cases of _gradient_descent's rule, by hand."""
    y = np.array([[1.0, 2.0], [3.0, 4.0]])
    update = np.array([[0.5, -0.5], [0.5, 0.0]])
    gains = np.array([[1.0, 1.0], [0.01, 2.0]])
    grad = np.array([[-2.0, -2.0], [1.0, 3.0]])
    y1, u1, g1, norm = O.update_rule(y, update, gains, grad, 0.5, 10.0)
    want_g = np.array([[1.2, 0.8], [0.01, 1.6]])  # inc, dec, dec clipped at 0.01, update == 0 is "dec"
    np.testing.assert_allclose(g1, want_g, rtol=1e-15)
    np.testing.assert_allclose(u1, 0.5 * update - 10.0 * want_g * grad, rtol=1e-15)
    np.testing.assert_allclose(y1, y + u1, rtol=1e-15)
    np.testing.assert_allclose(norm, np.linalg.norm(want_g * grad), rtol=1e-15)


def test_ops_symmetrize_on_cpu_tensors(gold, oracle_p):
    """ops.tsne_symmetrize is torch on whatever device its operands are on.
    Fed the fp32 conditional probabilities the oracle is fed, it has the same
    pattern, and its fp32 values are the oracle's float64 ones rounded once
    (2^-24 relative) after float64 sums that differ in order only (~1e-16):
    2^-23 relative bounds both."""
    p32 = oracle_p[0].astype(np.float32)
    row_ptr, col, val = ops.tsne_symmetrize(torch.from_numpy(gold["nn_idx"]), torch.from_numpy(p32))
    assert row_ptr.dtype == col.dtype == torch.int32 and val.dtype == torch.float32
    o_ptr, o_col, o_val = O.to_csr(O.symmetrize(gold["nn_idx"], p32))
    assert np.array_equal(row_ptr.numpy(), o_ptr) and np.array_equal(col.numpy(), o_col)
    assert np.abs(val.numpy().astype(np.float64) - o_val).max() <= 2.0 ** -23 * o_val.max()
    assert (np.abs(val.numpy().astype(np.float64) - o_val) <= 2.0 ** -23 * o_val).all()
    for i in (0, 57, 199):  # columns ascending within a row
        c = col[row_ptr[i]:row_ptr[i + 1]].numpy()
        assert (np.diff(c) > 0).all() and i not in c


def test_ops_symmetrize_hand_case_and_refusals():
    idx = torch.tensor([[1], [0], [0]], dtype=torch.int32)  # 0 <-> 1 mutual, 2 -> 0 one-sided
    p = torch.tensor([[1.0], [1.0], [1.0]])
    row_ptr, col, val = ops.tsne_symmetrize(idx, p)
    assert row_ptr.tolist() == [0, 2, 3, 4] and col.tolist() == [1, 2, 0, 0]
    np.testing.assert_allclose(val.numpy(), np.array([2, 1, 2, 1]) / 6.0, rtol=2.0 ** -23)
    row_ptr, col, val = ops.tsne_symmetrize(idx, torch.tensor([[1.0], [1.0], [0.0]]))  # a zero entry drops out
    assert row_ptr.tolist() == [0, 1, 2, 2] and col.tolist() == [1, 0]
    with pytest.raises(ValueError):
        ops.tsne_symmetrize(torch.tensor([[3], [0], [0]], dtype=torch.int32), p)  # index outside [0, n)
    with pytest.raises(ValueError):
        ops.tsne_symmetrize(torch.tensor([[1, 1], [0, 2], [0, 1]], dtype=torch.int32), torch.ones(3, 2))  # twice
    with pytest.raises(ValueError):
        ops.tsne_symmetrize(idx, torch.ones(3, 2))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


def _refused(lib, rc, word, code=-1):
    assert rc == code and word in lib.cfsd_last_error_string(), (rc, lib.cfsd_last_error_string())


def test_abi_version_and_constants(lib):
    # the issue's "at least 4.20"; 4.20 was taken when this was built, so the t-SNE entry points are 4.21
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 21
    for name in ("cfsd_knn_rows", "cfsd_knn_rows_workspace", "cfsd_tsne_affinities", "cfsd_tsne_splits",
                 "cfsd_tsne_step_workspace", "cfsd_tsne_forces", "cfsd_tsne_update"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert ops.TSNE_MAX_D == 512 and ops.TSNE_MAX_K >= 91
    assert ops.TSNE_ROWS % ops.TSNE_TILE == 0


def test_knn_rows_validates_before_any_hip_call(lib):
    p, z = ctypes.c_void_p(16), ctypes.c_size_t(0)
    big = ops.TSNE_MAX_K
    _refused(lib, lib.cfsd_knn_rows(None, p, p, None, z, 10, 3, 2, None), b"null")
    _refused(lib, lib.cfsd_knn_rows(p, None, p, None, z, 10, 3, 2, None), b"null")
    _refused(lib, lib.cfsd_knn_rows(p, p, None, None, z, 10, 3, 2, None), b"null")
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 1, 3, 1, None), b"at least 2")       # n < 2
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 10, 3, 0, None), b"k=0")              # k = 0
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 10, 3, 10, None), b"k=10")            # k > n - 1
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 1000, 3, big + 1, None), b"k=")       # k > CFSD_TSNE_MAX_K
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 10, 0, 2, None), b"d=0")              # d = 0
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 10, 513, 2, None), b"d=513")          # d > 512
    _refused(lib, lib.cfsd_knn_rows(p, p, p, None, z, 2 ** 31 // big, 3, big, None), b"2^31")  # n * k = 2^31
    assert lib.cfsd_knn_rows_workspace(50000, 75, 91) == 0


def test_tsne_affinities_validates_before_any_hip_call(lib):
    p, big = ctypes.c_void_p(16), ops.TSNE_MAX_K
    _refused(lib, lib.cfsd_tsne_affinities(None, p, p, 10, 2, 5.0, None), b"null")
    _refused(lib, lib.cfsd_tsne_affinities(p, None, p, 10, 2, 5.0, None), b"null")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, None, 10, 2, 5.0, None), b"null")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 1, 1, 5.0, None), b"at least 2")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 10, 0, 5.0, None), b"k=0")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 10, 10, 5.0, None), b"k=10")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 1000, big + 1, 5.0, None), b"k=")
    _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 2 ** 31 // big, big, 5.0, None), b"2^31")
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        _refused(lib, lib.cfsd_tsne_affinities(p, p, p, 10, 2, bad, None), b"perplexity")


def test_tsne_step_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(16)
    need = lib.cfsd_tsne_step_workspace(700, 3)
    # forces [n][4] fp32, three float64 per attraction workgroup, partials [S][n][3] fp32
    assert need == 700 * 16 + -(-700 // ops.TSNE_ATT_ROWS) * 24 + 3 * 700 * 12
    assert lib.cfsd_tsne_step_workspace(700, 0) == lib.cfsd_tsne_step_workspace(700, lib.cfsd_tsne_splits(700))
    assert lib.cfsd_tsne_step_workspace(1, 1) == 0 and lib.cfsd_tsne_step_workspace(700, ops.TSNE_MAX_SPLITS + 1) == 0
    ws = ctypes.c_size_t(need)
    _refused(lib, lib.cfsd_tsne_forces(None, p, p, p, p, ws, 700, 9, 3, 1.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_forces(p, None, p, p, p, ws, 700, 9, 3, 1.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_forces(p, p, None, p, p, ws, 700, 9, 3, 1.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, None, p, ws, 700, 9, 3, 1.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, None, ws, 700, 9, 3, 1.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ws, 1, 9, 3, 1.0, 0, None), b"n=1")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ws, 700, -1, 3, 1.0, 0, None), b"nnz")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ws, 700, 9, -1, 1.0, 0, None), b"splits")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ws, 700, 9, ops.TSNE_MAX_SPLITS + 1, 1.0, 0, None), b"splits")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ws, 700, 9, 3, 0.0, 0, None), b"exaggeration")
    _refused(lib, lib.cfsd_tsne_forces(p, p, p, p, p, ctypes.c_size_t(need - 1), 700, 9, 3, 1.0, 0, None),
             b"workspace", code=-2)
    _refused(lib, lib.cfsd_tsne_update(None, p, p, p, p, p, ws, 700, 3, 1.0, 0.5, 50.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_update(p, None, p, p, p, p, ws, 700, 3, 1.0, 0.5, 50.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_update(p, p, None, p, p, p, ws, 700, 3, 1.0, 0.5, 50.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_update(p, p, p, None, p, p, ws, 700, 3, 1.0, 0.5, 50.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_update(p, p, p, p, None, p, ws, 700, 3, 1.0, 0.5, 50.0, 1, None), b"null")  # result
    _refused(lib, lib.cfsd_tsne_update(p, p, p, p, p, None, ws, 700, 3, 1.0, 0.5, 50.0, 0, None), b"null")
    _refused(lib, lib.cfsd_tsne_update(p, p, p, p, p, p, ws, 1, 3, 1.0, 0.5, 50.0, 0, None), b"n=1")
    _refused(lib, lib.cfsd_tsne_update(p, p, p, p, p, p, ws, 700, 65, 1.0, 0.5, 50.0, 0, None), b"splits")
    _refused(lib, lib.cfsd_tsne_update(p, p, p, p, p, p, ctypes.c_size_t(8), 700, 3, 1.0, 0.5, 50.0, 0, None),
             b"workspace", code=-2)


def test_auto_splits_is_a_function_of_n(lib):
    """ceil(2048 / row blocks), at most one split per column tile and CFSD_TSNE_MAX_SPLITS."""
    for n in (2, 127, 128, 129, 512, 513, 2048, 8192, 32768, 50000):
        blocks, tiles = -(-n // ops.TSNE_ROWS), -(-n // ops.TSNE_TILE)
        assert ops.tsne_splits(n) == min(-(-2048 // blocks), tiles, ops.TSNE_MAX_SPLITS)


def test_ops_reject_host_tensors_and_bad_arguments():
    z = torch.zeros(10, 3)
    with pytest.raises(ValueError, match="device tensor"):
        ops.knn_rows(z, 2)
    with pytest.raises(ValueError, match="device tensor"):
        ops.tsne_affinities(torch.zeros(10, 2), 5.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.tsne_joint_probabilities(z, 2.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.tsne_step(torch.zeros(10, 2), torch.zeros(10, 2), torch.ones(10, 2),
                      (torch.zeros(11, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0)), 0.5, 50.0)
    with pytest.raises(ValueError, match="device tensor"):
        tsne.fit_transform(z)


def test_perplexity_not_below_n_is_a_value_error():
    """scikit-learn's own check (TSNE._check_params_vs_input) and message."""
    for perplexity in (10.0, 11.5):
        with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
            ops.tsne_joint_probabilities(torch.zeros(10, 3), perplexity)
    with pytest.raises(ValueError, match="positive"):
        ops.tsne_joint_probabilities(torch.zeros(10, 3), 0.0)


def test_tester_has_a_tsne_step_and_embeddings_still_refuses(tmp_path):
    assert "tsne" in evaluation.Tester.STEPS
    stats = {k: torch.zeros(4) for k in ("means", "stds", "mins", "maxs")}
    manager = types.SimpleNamespace(net=types.SimpleNamespace(eval=lambda: None), device=torch.device("cpu"),
                                    is_vae=True, bs=2, latent_regions={})
    config = {"data": {"normalize_data": False}, "model": {"latent_size": 4}}
    t = evaluation.Tester(manager, None, None, None, str(tmp_path), config, latent_stats=stats)
    with pytest.raises(NotImplementedError, match="tsne_embeddings"):
        t.embeddings(mode="tsne")
    assert callable(t.tsne_embeddings)
    with pytest.raises(ValueError):
        t.run("t-sne")
