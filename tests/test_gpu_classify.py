"""The classifier stage on the GPU (``csrc/classify.hip``, ``classify.py``;
reference ``model_manager.py:403-573``, ``model.py:191-203``).

References: scikit-learn's LDA / QDA outputs recorded by
``golden/make_classify.py`` on the seeded inputs of ``golden/classify_cases.py``
(regenerated here from the seed), float64 NumPy restatements of the statistics
and of the Mahalanobis distance, and -- for the MLP -- the reference's own
module (``nn.Sequential`` of ``Linear + ReLU``) with ``CrossEntropyLoss(weight)``
and ``torch.optim.Adam`` on the CPU in float64.

Bounds.  Statistics and scores: the project's standing fp32 bound, 1e-4 of the
largest reference value (a NumPy fp32 restatement of the pipeline is 1e-6 to
5e-6 off on these inputs); means 1e-6 absolute (compensated sums).  MLP: see
``test_mlp_train_steps``.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

import cfsd_loader
import classify_cases as cases
import recipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cfsd_loader.load()
from craniofacialsd_vae_amd import classify as C  # noqa: E402
from craniofacialsd_vae_amd import ops  # noqa: E402

CASE_NAMES = list(cases.CASES)


@pytest.fixture(scope="module")
def sk():
    return np.load(os.path.join(recipe.HERE, "classify_sklearn.npz"))


@pytest.fixture(scope="module")
def case_data():
    """Per case: the inputs, their float64 statistics, and the device copies."""
    out = {}
    for name in CASE_NAMES:
        case = cases.make_case(name)
        x, y = cases.valid_rows(case)
        n_cls = case["n_classes"]
        count = np.array([(y == c).sum() for c in range(n_cls)])
        mean = np.stack([x[y == c].mean(0) for c in range(n_cls)])
        scatter = np.stack([(x[y == c] - mean[c]).T @ (x[y == c] - mean[c]) for c in range(n_cls)])
        out[name] = dict(case, count=count, mean=mean, scatter=scatter, z_dev=torch.from_numpy(case["z"]).cuda(),
                         y_dev=torch.from_numpy(case["y"]).cuda(), zt_dev=torch.from_numpy(case["zt"]).cuda())
    return out


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("name", CASE_NAMES)
def test_class_stats(case_data, name):
    """Counts exact, means within 1e-6, scatter within 1e-4 max|S_c| of
    float64; a second call gives the same bits.  full75 spans two row slices,
    region5 reads the window [70, 75) of 75 columns, odd20 carries a row whose
    label is out of range."""
    d = case_data[name]
    got = ops.class_stats(d["z_dev"], d["y_dev"], d["n_classes"], d["cols"])
    count, mean, scatter = (t.cpu().numpy() for t in got)
    assert np.array_equal(count, d["count"])
    err_mean = np.abs(mean - d["mean"]).max()
    err_s = max(np.abs(scatter[c] - d["scatter"][c]).max() / np.abs(d["scatter"][c]).max()
                for c in range(d["n_classes"]))
    print(f"{name}: mean err {err_mean:.2e}, scatter err {err_s:.2e} of max|S_c|")
    assert err_mean <= 1e-6
    assert err_s <= 1e-4
    again = ops.class_stats(d["z_dev"], d["y_dev"], d["n_classes"], d["cols"])
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_class_stats_refuses_bad_shapes():
    z = torch.zeros(8, 130, device="cuda")
    y = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.class_stats(z, y, 2)                 # 130 columns > 128
    with pytest.raises(ValueError):
        ops.class_stats(z, y, 65, cols=(0, 5))   # 65 classes > 64
    with pytest.raises(ValueError):
        ops.class_stats(z, y, 2, cols=(128, 5))  # window past the row
    with pytest.raises(ValueError):              # a class with fewer than 2 rows
        C.QuadraticDiscriminant("cuda").fit(torch.randn(5, 3, device="cuda"), torch.tensor([0, 0, 0, 1, 0]))


# ---------------------------------------------------------------- LDA / QDA
def _row_centred(a):
    return a - a.mean(1, keepdims=True)


def _check_scores(got, ref, pred, ref_pred, what):
    """Scores within 1e-4 max|ref|; labels equal on every row whose reference
    top-two margin exceeds twice that; at most 2 % of rows excluded."""
    tol = 1e-4 * np.abs(ref).max()
    err = np.abs(got - ref).max()
    top = np.sort(ref, axis=1)
    sure = (top[:, -1] - top[:, -2]) > 2 * tol
    print(f"{what}: score err {err / np.abs(ref).max():.2e} of max|score|, {int((~sure).sum())} rows within the margin")
    assert err <= tol
    assert (~sure).mean() <= 0.02
    assert np.array_equal(pred[sure], ref_pred[sure])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_qda_matches_sklearn(case_data, sk, name):
    d = case_data[name]
    qda = C.QuadraticDiscriminant("cuda").fit(d["z_dev"], d["y_dev"], cols=d["cols"], n_classes=d["n_classes"])
    np.testing.assert_allclose(qda.means_, sk[f"{name}.qda_means"], atol=1e-6)
    np.testing.assert_allclose(qda.priors_, sk[f"{name}.qda_priors"], rtol=1e-12)
    dec = qda.decision_function(d["zt_dev"]).cpu().numpy()
    pred = qda.predict(d["zt_dev"]).cpu().numpy()
    _check_scores(dec, sk[f"{name}.qda_decision"], pred, sk[f"{name}.qda_pred"], f"{name} qda")
    assert abs(qda.score(d["zt_dev"], d["yt"]) - (sk[f"{name}.qda_pred"] == d["yt"]).mean()) <= 0.02
    # Mahalanobis distance to every class: sqrt((z - m) S^-1 (z - m)) in float64
    col0, w = d["cols"]
    xt = d["zt"][:, col0:col0 + w].astype(np.float64)
    ref = np.stack([np.sqrt(np.einsum("ij,jk,ik->i", xt - d["mean"][c],
                                      np.linalg.inv(d["scatter"][c] / (d["count"][c] - 1)), xt - d["mean"][c]))
                    for c in range(d["n_classes"])], 1)
    got = torch.sqrt(qda.mahalanobis2(d["zt_dev"])).cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-4 * ref.max()
    # tensors-only persistence: a reloaded classifier scores the same bits
    sd = {k: v.clone() for k, v in qda.state_dict().items()}
    assert all(torch.is_tensor(v) for v in sd.values())
    again = C.QuadraticDiscriminant("cuda").load_state_dict(sd)
    assert torch.equal(again.decision_function(d["zt_dev"]), qda.decision_function(d["zt_dev"]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_lda_matches_sklearn(case_data, sk, name):
    """Decision values up to scikit-learn's per-row constant (row-centred),
    log-posteriors, labels, and the 2-D transform up to one sign per
    component, all within 1e-4 of the largest reference value."""
    d = case_data[name]
    lda = C.LinearDiscriminant("cuda").fit(d["z_dev"], d["y_dev"], cols=d["cols"], n_classes=d["n_classes"])
    np.testing.assert_allclose(lda.means_, sk[f"{name}.lda_means"], atol=1e-6)
    dec = lda.decision_function(d["zt_dev"]).cpu().numpy()
    pred = lda.predict(d["zt_dev"]).cpu().numpy()
    _check_scores(_row_centred(dec), _row_centred(sk[f"{name}.lda_decision"]), pred, sk[f"{name}.lda_pred"],
                  f"{name} lda")
    logp, ref = lda.predict_log_proba(d["zt_dev"]).cpu().numpy(), sk[f"{name}.lda_log_proba"]
    assert np.abs(logp - ref).max() <= 1e-4 * np.abs(ref).max()
    tr, ref = lda.transform(d["zt_dev"]).cpu().numpy(), sk[f"{name}.lda_transform"]
    assert tr.shape == ref.shape == (len(d["zt"]), 2)
    sign = np.sign((tr * ref).sum(0))
    assert np.abs(tr * sign - ref).max() <= 1e-4 * np.abs(ref).max()
    cov = sum(d["count"][c] / d["count"].sum() * d["scatter"][c] / d["count"][c] for c in range(d["n_classes"]))
    np.testing.assert_allclose(lda.covariance_, cov, atol=1e-4 * np.abs(cov).max())


def test_discriminant_tie_takes_lower_class():
    """Two identical classes (1 and 2): bit-equal scores, the lower index wins."""
    g = torch.Generator().manual_seed(3)
    d = 7
    m = torch.randn(1, d, generator=g)
    mean = torch.cat([m + 50.0, m, m]).cuda().contiguous()
    w = torch.randn(1, d, d, generator=g).cuda()
    offset = torch.tensor([0.3, -0.2, -0.2]).cuda()
    z = (torch.randn(130, d, generator=g) + m).cuda()
    for whiten in (w, w.repeat(3, 1, 1).contiguous()):
        out = ops.discriminant_scores(z, mean, whiten, offset, want_maha2=True)
        assert torch.equal(out["scores"][:, 1], out["scores"][:, 2])
        assert torch.all(out["pred"] == 1)
        ref = (((z - mean[1]).double() @ whiten[0].double()) ** 2).sum(1)
        assert torch.allclose(out["maha2"][:, 1].double(), ref, rtol=1e-4)


# ---------------------------------------------------------------- MLP
MLP_CASES = {
    # name: (dims, bs, N, lr, n for the forward test)
    "craniofacial": ([75, 512, 128, 64, 4], 4, 48, 1e-4, 37),
    "odd": ([10, 33, 17, 3], 3, 22, 1e-3, 5),   # one row left over, never visited
}


class RefMLP(nn.Module):
    """The reference's MLPClassifier (model.py:191-203), restated."""

    def __init__(self, dims):
        super().__init__()
        layers = []
        for i in range(1, len(dims)):
            layers += [nn.Linear(dims[i - 1], dims[i]), nn.ReLU()]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        out = self.model(x)
        return out, torch.max(torch.log_softmax(out, dim=1), dim=1)[1]


def _flat(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()])


def _mlp_setup(name, seed=5):
    dims, bs, n, lr, n_fwd = MLP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(max(n, n_fwd), dims[0], generator=g)
    y = torch.randint(0, dims[-1], (n,), generator=g, dtype=torch.int32)
    counts = np.bincount(y.numpy(), minlength=dims[-1]).astype(np.float64) + 1
    w = torch.from_numpy((1 / counts / (1 / counts).sum()).astype(np.float32))
    mlp = C.MLPClassifier(dims[0], dims[1:-1], dims[-1], device="cuda", seed=seed, lr=lr)
    ref = RefMLP(dims).double()
    ref.load_state_dict({k: v.cpu().double() for k, v in mlp.state_dict().items()})
    return dims, bs, n, lr, n_fwd, z, y, w, mlp, ref


@pytest.fixture(scope="module")
def mlp_reference():
    """Float64 CPU training of both MLP cases: 3 epochs of the reference's
    mlp_classifier_epoch.  Computed once; read-only."""
    out = {}
    for name in MLP_CASES:
        dims, bs, n, lr, _, z, y, w, mlp, ref = _mlp_setup(name)
        opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=0.0)
        crit = nn.CrossEntropyLoss(w.double())
        first_grad, epochs = None, []
        for _ in range(3):
            loss_sum = acc_sum = 0.0
            for t in range(n // bs):
                zb, yb = z[t * bs:(t + 1) * bs].double(), y[t * bs:(t + 1) * bs].long()
                opt.zero_grad()
                o, lab = ref(zb)
                loss = crit(o, yb)
                loss.backward()
                if first_grad is None:
                    first_grad = torch.cat([p.grad.reshape(-1) for p in ref.parameters()]).clone()
                opt.step()
                loss_sum += loss.item()
                acc_sum += 100.0 * (np.argmax(o.detach().numpy(), 1) == yb.numpy()).sum() / bs
            epochs.append((loss_sum / (n // bs), acc_sum / (n // bs)))
        out[name] = {"first_grad": first_grad.numpy(), "epochs": epochs, "params": _flat(ref).numpy()}
    return out


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_forward(name):
    """Logits of one launch against the float64 module, within 1e-4 of the
    largest; labels = arg max of the kernel's own logits, lowest index."""
    dims, _, _, _, n_fwd, z, _, _, mlp, ref = _mlp_setup(name)
    out, lab = mlp(z[:n_fwd].cuda())
    with torch.no_grad():
        r = ref(z[:n_fwd].double())[0].numpy()
    got = out.cpu().numpy()
    assert got.shape == (n_fwd, dims[-1]) and got.min() >= 0  # a ReLU after the last layer too
    assert np.abs(got - r).max() <= 1e-4 * np.abs(r).max()
    assert np.array_equal(lab.cpu().numpy(), np.argmax(got, 1))


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_train_steps(mlp_reference, name):
    """3 epochs against float64 torch (CrossEntropyLoss(weight) + Adam).
    First-step gradient (dw_out) within 1e-4 by max|g - r| / (1 + max|r|);
    per-epoch mean loss rtol 1e-4, accuracy exact; parameters after the last
    step within 1e-5 absolute (fp32 torch is 1.4e-7 from float64 torch on
    these runs, and one wrongly signed Adam update would be >= lr = 1e-4).
    Observed on an MI355X: first gradient 7.5e-9 / 7.1e-9, epoch loss 9.4e-8 /
    1.3e-7 relative, parameters 5.2e-8 / 1.2e-7 (craniofacial / odd case).
    "Exact" accuracy: the same number of correct rows in every epoch -- one row
    is worth 100 / (bs steps) >= 2.08 points, the fp32 sum of the per-step
    percentages is within steps x ulp(100) ~ 1e-4 of the float64 one, so the
    comparison allows 1e-3.
    A second run gives the same bits; a validation epoch (train=False) leaves
    parameters, moments and step untouched and returns the forward's loss."""
    dims, bs, n, lr, _, z, y, w, mlp, _ = _mlp_setup(name)
    R = mlp_reference[name]
    zd, yd, wd = z[:n].cuda(), y.cuda(), w.cuda()
    probe = _mlp_setup(name)[8]  # the same initial parameters: one step, its gradient kept
    dw = torch.full_like(probe.flat, float("nan"))
    ops.mlp_train_steps(zd, yd, wd, probe.flat, probe.exp_avg, probe.exp_avg_sq, probe.step, probe._acc, dims, bs, 1,
                        lr=lr, dw_out=dw)
    g = dw.cpu().numpy()
    err_g = np.abs(g - R["first_grad"]).max() / (1 + np.abs(R["first_grad"]).max())
    assert int(probe.step.item()) == 1
    epochs = [mlp.run_epoch(zd, yd, wd, bs, train=True) for _ in range(3)]
    assert int(mlp.step.item()) == 3 * (n // bs)
    err_p = np.abs(mlp.flat.cpu().numpy() - R["params"]).max()
    err_l = max(abs(a[0] - b[0]) / abs(b[0]) for a, b in zip(epochs, R["epochs"]))
    print(f"{name}: first gradient err {err_g:.2e}, epoch loss rel err {err_l:.2e}, parameter err {err_p:.2e}")
    assert err_g < 1e-4
    for (loss, acc), (rl, ra) in zip(epochs, R["epochs"]):
        assert abs(loss - rl) <= 1e-4 * abs(rl)
        assert abs(acc - ra) <= 1e-3
    assert err_p <= 1e-5
    # bit-identical second run
    other = _mlp_setup(name)[8]
    epochs2 = [other.run_epoch(zd, yd, wd, bs, train=True) for _ in range(3)]
    assert epochs2 == epochs and torch.equal(other.flat, mlp.flat) and torch.equal(other.exp_avg_sq, mlp.exp_avg_sq)
    # validation epoch
    before = [t.clone() for t in (mlp.flat, mlp.exp_avg, mlp.exp_avg_sq, mlp.step)]
    v_loss, v_acc = mlp.run_epoch(zd, yd, wd, bs, train=False)
    for a, b in zip(before, (mlp.flat, mlp.exp_avg, mlp.exp_avg_sq, mlp.step)):
        assert torch.equal(a, b)
    used = (n // bs) * bs
    o = mlp(zd[:used])[0].cpu().double()
    crit = nn.CrossEntropyLoss(w.double())
    ref_loss = np.mean([crit(o[t:t + bs], y[t:t + bs].long()).item() for t in range(0, used, bs)])
    ref_acc = np.mean([100.0 * (o[t:t + bs].argmax(1) == y[t:t + bs].long()).sum().item() / bs
                       for t in range(0, used, bs)])
    assert abs(v_loss - ref_loss) <= 1e-5 * abs(ref_loss)
    assert abs(v_acc - ref_acc) <= 1e-3


def test_mlp_dead_output_layer():
    """Last layer: weights 0, bias strongly negative -> every logit is 0 after
    the ReLU: pred 0, loss log C, all gradients 0, parameters unchanged and
    finite after a step (no 0/0 in Adam)."""
    dims, bs = [10, 33, 17, 3], 3
    mlp = C.MLPClassifier(dims[0], dims[1:-1], dims[-1], device="cuda", seed=2, lr=1e-3)
    mlp.model[4].weight.data.zero_()
    mlp.model[4].bias.data.fill_(-5.0)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(6, dims[0], generator=g).cuda()
    y = torch.tensor([0, 1, 2, 2, 1, 0], dtype=torch.int32).cuda()
    w = torch.tensor([0.5, 0.3, 0.2]).cuda()
    out, lab = mlp(z)
    assert torch.all(out == 0) and torch.all(lab == 0)
    before = mlp.flat.clone()
    dw = torch.full_like(mlp.flat, float("nan"))
    loss, acc = mlp.run_epoch(z, y, w, bs, train=True, dw_out=dw)
    assert loss == pytest.approx(np.log(3), rel=1e-6)
    assert acc == pytest.approx(100.0 * 2 / 6, abs=1e-3)
    assert torch.all(dw == 0)
    assert torch.equal(mlp.flat, before) and torch.isfinite(mlp.flat).all()
    assert torch.all(mlp.exp_avg == 0) and torch.all(mlp.exp_avg_sq == 0) and int(mlp.step.item()) == 2


# ---------------------------------------------------------------- driver
CONFIG = {
    "optimization": {"epochs": 2, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
    "classifier": {"main_model_type": "qda", "mlp_training_type": "after", "mlp_hidden_features": [32, 16],
                   "mlp_lr": 1e-3, "mlp_epochs": 2},
    "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
}


@pytest.fixture(scope="module")
def trained(tmp_path_factory, topo_npz):
    """The demo workspace (40 OBJ files, classes n / a / c / m) trained for 2
    epochs through the driver with a ``classifier:`` section."""
    from craniofacialsd_vae_amd import precompute
    from craniofacialsd_vae_amd import train as T
    d = tmp_path_factory.mktemp("demo_cls")
    precompute.write_ply(str(d / "template.ply"), topo_npz["pos_0"], topo_npz["face_0"], topo_npz["template_colors"])
    (d / "pre").mkdir()
    np.savez(d / "pre" / "topology.npz", **topo_npz)
    (d / "meshes").mkdir()
    m = recipe.load_meshes()
    rs = np.random.RandomState(3)
    for i in range(40):
        v = m["verts"][i % 12] + (0 if i < 12 else rs.normal(0, 0.002, m["verts"][0].shape))
        with open(d / "meshes" / f"{'nacm'[i % 4]}_{i:03d}.obj", "w") as f:
            for p in v.astype(np.float32):
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": 89.11,
                             "swap_features": True, "stratified_split": False})
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    manager, _ = T.main(["--config", str(d / "config.yaml"), "--id", "cls", "--output_path", str(d / "runs")])
    return d, cfg, manager, d / "runs" / "outputs" / "cls"


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_driver_trains_and_resumes_classifiers(trained):
    """(The demo split is not stratified: its 28 training rows hold the
    classes c / m / n only, 9-10 rows each at d = 75, so the discriminants are
    fitted on three classes and rank-deficient, which exercises the
    eigenvalue floor; the numbers are checked above.)"""
    from craniofacialsd_vae_amd import data as D
    from craniofacialsd_vae_amd import manager as M
    d, cfg, man, od = trained
    assert sorted(os.listdir(od / "checkpoints")) == [
        "lda_classifier.pt", "mlp_classifier.pt", "model_00000001.pt", "model_00000002.pt", "optimizer.pt",
        "qda_classifier.pt", "region_ldas.pt", "region_qdas.pt"]
    acc = json.load(open(od / "classifiers.json"))["validation_accuracy"]
    assert sorted(acc) == ["lda", "mlp", "qda"] and all(0 <= acc[k] <= 100 for k in acc)
    logs = [json.loads(ln) for ln in open(od / "logs" / "scalars.jsonl")]
    cls = [(x["tag"], x["step"]) for x in logs if "class_" in x["tag"]]
    assert sorted(cls) == sorted((f"{ph}/class_{k}", e) for ph in ("train", "validation") for k in ("loss", "acc")
                                 for e in (1, 2))
    assert man.class2idx_dict == {"a": 0, "c": 1, "m": 2, "n": 3}
    assert man.qda.classes_.tolist() == [1, 2, 3] and float(man._class_weights[0]) == 0.0
    for name in ("lda_classifier.pt", "qda_classifier.pt", "region_ldas.pt", "region_qdas.pt"):
        torch.load(od / "checkpoints" / name, weights_only=True)  # tensors only: no pickled objects
    # a fresh manager resumes the same classifiers
    fresh = M.ModelManager(cfg, device="cuda", precomputed_storage_path=cfg["data"]["precomputed_path"],
                           use_graph=False)
    assert fresh.resume(str(od / "checkpoints")) == 2
    tr, va, te, norm = D.load_mesh_dataset(cfg["data"], 4, "cuda")
    z = man.encode(te.meshes)
    assert torch.equal(fresh.encode(te.meshes), z)
    region = list(man.latent_regions)[-1]
    for model in ("main", "mlp", "lda", "qda"):
        labels = man.classify_latent(z, model)
        assert labels == fresh.classify_latent(z, model) and set(labels) <= set("acmn") and len(labels) == len(z)
        assert model == "mlp" or "a" not in labels  # no training mesh of class a: never a discriminant's answer
    for reg in ("all", region):
        a = man.mahalanobis_dist_to_qda_distribution(z, "n", reg)
        assert a.shape == (len(z),) and torch.isfinite(a).all()
        assert torch.equal(a, fresh.mahalanobis_dist_to_qda_distribution(z, "n", reg))
    assert torch.equal(man.lda_project_latents_in_2d(z), fresh.lda_project_latents_in_2d(z))
    s = man.qda_sample("n", 5, generator=torch.Generator(device="cuda").manual_seed(1))
    assert s.shape == (5, 75) and torch.isfinite(s).all()
    # mlp_classifier.pt is the reference's format: it loads into the reference-shaped module
    ref = RefMLP([75, 32, 16, 4])
    ref.load_state_dict(torch.load(od / "checkpoints" / "mlp_classifier.pt", weights_only=True)["model"])
    with torch.no_grad():
        r = ref(z.cpu())[0].numpy()
    got = man.classifier_mlp(z)[0].cpu().numpy()
    assert np.abs(got - r).max() <= 1e-4 * max(np.abs(r).max(), 1e-30)
    # ... and in the other direction
    other = C.MLPClassifier(75, [32, 16], 4, device="cuda", seed=9)
    other.load_state_dict(ref.state_dict())
    assert torch.equal(other.flat, man.classifier_mlp.flat)
