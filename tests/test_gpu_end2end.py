"""``classifier.mlp_training_type: end2end`` on the GPU: the MLP classifier as
a head of the VAE step (``cfsd_mlp_head_step``, ``SDVAEEngine.
attach_classifier_head``, ``step.TrainStep``, ``manager.ModelManager``;
reference ``model_manager.py:295-318, 457, 682-735``).

References.  Per op: the reference's module in float64 torch (``RefMLP``),
``CrossEntropyLoss(weight)`` and autograd w.r.t. ``z``.  Full step: the CPU
oracle's ``losses`` plus ``w_cls * CE(ref(z[diagonal]), y)``, autograd, and two
``O.Adam`` (the VAE's and, with ``mlp_lr``, the classifier's).

Bounds.  Per op: the project's ``close(..., 1e-5)``; accuracy within 1e-3 (one
row is worth 100 / bs >= 6.25 points; the argument of
``test_gpu_classify.test_mlp_train_steps``); parameters after one Adam step
within 1e-5 absolute at lr = 1e-4, the reference's ``mlp_lr`` and that test's:
a wrongly signed update is off by 2 lr = 2e-4.  (Adam's first update is
lr g / (|g| + 1e-8): where |g| is near 1e-8 it amplifies the gradient's fp32
rounding by up to lr / 4e-8.  fp32 torch on the CPU is 6.0e-7 from float64
torch on case a at lr = 1e-4 and 6.0e-6 at 1e-3, on an element with g =
8.2e-9; at 1e-3 the format's own error would fill the bound, so 1e-3 is not
used.)
Full step: ``test_gpu_parity.test_train_three_steps_golden``'s (losses rtol
1e-4, gradients close 1e-4, parameters 2e-5), accuracy exact.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

import cfsd_loader
import recipe
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cfsd_loader.load()
from craniofacialsd_vae_amd import classify as C  # noqa: E402
from craniofacialsd_vae_amd import engine as E  # noqa: E402
from craniofacialsd_vae_amd import ops, topology  # noqa: E402
from craniofacialsd_vae_amd.step import TrainStep  # noqa: E402

DEV = "cuda"


def close(a, b, rel=1e-5, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    tol = rel * (1.0 + np.abs(b).max())
    err = np.abs(a - b).max()
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"


class RefMLP(nn.Module):
    """The reference's MLPClassifier (model.py:191-203), restated."""

    def __init__(self, dims):
        super().__init__()
        layers = []
        for i in range(1, len(dims)):
            layers += [nn.Linear(dims[i - 1], dims[i]), nn.ReLU()]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def ref_of(mlp, dtype=torch.float32):
    ref = RefMLP(mlp.dims).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in mlp.state_dict().items()})
    return ref


def flat_grad(ref):
    return torch.cat([p.grad.reshape(-1) for p in ref.parameters()])


@pytest.fixture(scope="module")
def dtopo(topo_npz):
    return topology.DeviceTopology.from_npz(topo_npz, device=DEV)


# ---------------------------------------------------------------- per op
HEAD_CASES = {
    # name: (dims, bs, row_stride, rows of z / dlat)
    "a": ([75, 512, 128, 64, 3], 4, 5, 16),     # the craniofacial head: the diagonal of a 4 x 4 group
    "b": ([33, 40, 7, 5], 3, 1, 3),             # odd widths, consecutive rows (swap_features: False)
    "c": ([75, 64, 4], 16, 17, 256),            # the largest batch: the 16-row tile, stride 17
}
LR = 1e-4
N_TABLE = 40


class HeadCase:
    """Inputs of one case and its float64 reference; device state rebuilt per run."""

    # seed 5: the first seed at which, in the float64 reference of all three cases, every row has a live
    # (positive) logit -- so every chosen row of dlat receives a gradient -- and the accuracy is neither 0 nor 100
    def __init__(self, name, seed=5):
        self.dims, self.bs, self.stride, self.rows = HEAD_CASES[name]
        d, c = self.dims[0], self.dims[-1]
        g = torch.Generator().manual_seed(seed)
        self.z = torch.randn(self.rows, d, generator=g)
        self.dlat0 = torch.randn(self.rows, 3 * d, generator=g)
        self.table = torch.randint(0, c, (N_TABLE,), generator=g, dtype=torch.int32)
        self.bidx = torch.randperm(N_TABLE, generator=g)[:self.bs].to(torch.int32)
        self.cw = torch.rand(c, generator=g) + 0.1
        self.cw = self.cw / self.cw.sum()
        self.sel = torch.arange(self.bs) * self.stride
        self.y = self.table[self.bidx.long()].long()
        self.seed = seed
        # float64 reference: loss, accuracy, d loss / dz, d loss / d parameters, parameters after Adam at w_cls
        ref = ref_of(self.fresh_mlp(), torch.float64)
        zs = self.z[self.sel].double().requires_grad_()
        out = ref(zs)
        loss = nn.CrossEntropyLoss(self.cw.double())(out, self.y)
        loss.backward()
        self.loss = loss.item()
        self.acc = 100.0 * (out.argmax(1) == self.y).sum().item() / self.bs
        self.dz = zs.grad.clone()
        assert (self.dz.abs().max(1)[0] > 0).all() and 0 < self.acc < 100
        self.grad = flat_grad(ref).clone()
        self.adam = {}
        for w in (1.0, 2.0):
            r = ref_of(self.fresh_mlp(), torch.float64)
            opt = torch.optim.Adam(r.parameters(), lr=LR, weight_decay=0.0)
            (w * nn.CrossEntropyLoss(self.cw.double())(r(self.z[self.sel].double()), self.y)).backward()
            opt.step()
            self.adam[w] = torch.cat([p.detach().reshape(-1) for p in r.parameters()])

    def fresh_mlp(self):
        return C.MLPClassifier(self.dims[0], self.dims[1:-1], self.dims[-1], device=DEV, seed=self.seed, lr=LR)

    def run(self, w_cls=1.0, train=True, adam=True):
        """One head step from the initial state; returns everything it may touch."""
        mlp = self.fresh_mlp()
        dlat = self.dlat0.to(DEV)
        acc = torch.zeros(3, device=DEV)
        dw = torch.full_like(mlp.flat, float("nan"))
        ops.mlp_head_step(self.z.to(DEV), self.bidx.to(DEV), self.table.to(DEV), self.cw.to(DEV), mlp.flat, acc,
                          self.dims, self.bs, row_stride=self.stride, train=train, m=mlp.exp_avg if adam else None,
                          v=mlp.exp_avg_sq if adam else None, step=mlp.step, dlat=dlat, w_cls=w_cls, dw_out=dw, lr=LR)
        torch.cuda.synchronize()
        return {"params": mlp.flat.cpu(), "m": mlp.exp_avg.cpu(), "v": mlp.exp_avg_sq.cpu(),
                "step": int(mlp.step.item()), "dlat": dlat.cpu(), "acc": acc.cpu().numpy(), "dw": dw.cpu(),
                "params0": self.fresh_mlp().flat.cpu()}


@pytest.fixture(scope="module")
def head_cases():
    return {name: HeadCase(name) for name in HEAD_CASES}


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_step_loss_and_dz(head_cases, name):
    """Loss, accuracy, and w_cls * dz added to the chosen rows of block 0 of a
    dlat of random values: the sum within 1e-5, every other element bit-equal."""
    hc = head_cases[name]
    d = hc.dims[0]
    for w in (1.0, 2.0):
        r = hc.run(w_cls=w, adam=False)
        print(f"{name} w_cls {w}: loss {r['acc'][0]:.7f} ref {hc.loss:.7f}, acc {r['acc'][1]} ref {hc.acc}")
        close(r["acc"][0], hc.loss, 1e-5, "loss")
        assert abs(r["acc"][1] - hc.acc) <= 1e-3 and r["acc"][2] == 1.0
        want = hc.dlat0.clone().double()
        want[hc.sel, :d] += w * hc.dz
        close(r["dlat"][hc.sel, :d], want[hc.sel, :d], 1e-5, "dlat + w_cls dz")
        # the term by itself (the difference of two fp32 values of size <= 5 carries <= 5e-7 of rounding)
        close(r["dlat"][hc.sel, :d].double() - hc.dlat0[hc.sel, :d].double(), w * hc.dz, 1e-5, "w_cls dz")
        touched = torch.zeros_like(hc.dlat0, dtype=torch.bool)
        touched[hc.sel, :d] = True
        assert torch.equal(r["dlat"][~touched], hc.dlat0[~touched])
        assert (r["dlat"][touched] != hc.dlat0[touched]).float().mean() > 0.5  # ... and the term did arrive


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_step_gradient_and_adam(head_cases, name):
    """Gradient-only mode: w_cls times the float64 gradient, parameters and
    moments untouched, the step counted.  Adam in place: the parameters after
    one step of torch's Adam on w_cls * loss, within 1e-5 absolute."""
    hc = head_cases[name]
    for w in (1.0, 2.0):
        r = hc.run(w_cls=w, adam=False)
        close(r["dw"], w * hc.grad, 1e-5, "parameter gradient")
        assert torch.equal(r["params"], r["params0"]) and r["step"] == 1
        assert torch.all(r["m"] == 0) and torch.all(r["v"] == 0)
        a = hc.run(w_cls=w, adam=True)
        assert torch.equal(a["dw"], r["dw"]) and torch.equal(a["dlat"], r["dlat"]) and a["step"] == 1
        err = (a["params"].double() - hc.adam[w]).abs().max().item()
        moved = (a["params"] != a["params0"]).float().mean().item()
        print(f"{name} w_cls {w}: parameters after Adam err {err:.2e}, {moved:.2f} of them moved")
        assert err <= 1e-5
        assert moved > 0.05  # (a dead ReLU leaves its incoming weights where they were)


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_step_validation_pass_writes_nothing(head_cases, name):
    hc = head_cases[name]
    r = hc.run(train=False)
    close(r["acc"][0], hc.loss, 1e-5, "loss")
    assert abs(r["acc"][1] - hc.acc) <= 1e-3 and r["acc"][2] == 1.0
    assert torch.equal(r["dlat"], hc.dlat0) and torch.equal(r["params"], r["params0"]) and r["step"] == 0
    assert torch.all(r["m"] == 0) and torch.all(r["v"] == 0) and torch.isnan(r["dw"]).all()


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_step_repeats_and_scales(head_cases, name):
    """A second run gives the same bits.  w_cls = 2 against w_cls = 1: the
    parameter gradient doubles exactly (a multiplication by 2 is exact); the dz
    term doubles within the rounding of the two sums: each of dlat + 1 dz and
    dlat + 2 dz is rounded once, to half an ulp of at most M = max|dlat after|,
    so (a2 - d0) - 2 (a1 - d0) is within 1.5 ulp(M) <= 1.5 * 2^-23 * M."""
    hc = head_cases[name]
    one, again, two = hc.run(1.0), hc.run(1.0), hc.run(2.0)
    for k in ("params", "m", "v", "dlat", "dw"):
        assert torch.equal(one[k], again[k]), k
    assert np.array_equal(one["acc"], again["acc"])
    assert torch.equal(two["dw"], 2 * one["dw"])
    d0 = hc.dlat0.double()
    diff = (two["dlat"].double() - d0) - 2 * (one["dlat"].double() - d0)
    big = max(one["dlat"].abs().max().item(), two["dlat"].abs().max().item())
    assert diff.abs().max().item() <= 1.5 * 2.0 ** -23 * big


def test_head_step_refuses_bad_shapes():
    dims = [8, 4, 3]
    n = ops.mlp_param_count(dims)
    f = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(ValueError):  # bs 17
        ops.mlp_head_step(f(17, 8), i(17), i(5), f(3), f(n), f(3), dims, 17, train=False)
    with pytest.raises(ValueError):  # width 1025
        ops.mlp_head_step(f(2, 8), i(2), i(5), f(3), f(n), f(3), [8, 1025, 3], 2, train=False)
    with pytest.raises(ValueError):  # 7 layers
        ops.mlp_head_step(f(2, 8), i(2), i(5), f(3), f(n), f(3), [8] * 7 + [3], 2, train=False)
    with pytest.raises(ValueError):  # the last strided row lies outside z
        ops.mlp_head_step(f(4, 8), i(2), i(5), f(3), f(n), f(3), dims, 2, row_stride=4, train=False)
    with pytest.raises(ValueError):  # a train step without moments or a gradient buffer
        ops.mlp_head_step(f(2, 8), i(2), i(5), f(3), f(n), f(3), dims, 2, step=i(1), dlat=f(2, 24))


# ---------------------------------------------------------------- full step vs the oracle
CLASS_W = [0.2, 0.5, 0.3]
LABELS = [0, 2, 1, 2]
MLP_SEED = 3
MLP_LR = 1e-3


def make_engine(dtopo, bs=4, precision="fp32", swap=True):
    eng = E.SDVAEEngine(dtopo, E.ModelSpec(), swap_bs=bs, device=DEV, precision=precision, swap_features=swap)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()})
    return eng


def make_head(eng, w_cls, hidden=(512, 128, 64)):
    mlp = C.MLPClassifier(75, list(hidden), 3, device=DEV, seed=MLP_SEED, lr=MLP_LR)
    eng.attach_classifier_head(mlp, torch.tensor(CLASS_W), w_cls, keep_grad=True)  # the tests read head.grad
    return mlp


def oracle_head_step(P, opt, Pc, optc, ref, x, otopo, key, eps, y, w_cls, diag, want_zero=True):
    """One _do_iteration with the classifier term on the CPU.  Returns the
    losses, the VAE gradients, the classifier's, and (want_zero) the encoder
    gradients of the same step without the term."""
    for p in list(P.values()) + list(Pc.values()):
        p.grad = None
    out = O.losses(P, x, otopo, key, torch.as_tensor(eps), bs=len(y))
    logits = ref(out["z"][diag])
    ce = nn.CrossEntropyLoss(torch.tensor(CLASS_W))(logits, torch.tensor(y))
    enc = [k for k in P if k.startswith("en_layers.")]
    g0 = dict(zip(enc, torch.autograd.grad(out["tot"], [P[k] for k in enc], retain_graph=True))) if want_zero else None
    tot = out["tot"] + w_cls * ce
    tot.backward()
    grads = {k: p.grad.detach().clone() for k, p in P.items()}
    gc = {k: p.grad.detach().clone() for k, p in Pc.items()}
    opt.step(P, grads)
    optc.step(Pc, gc)
    losses = [out[k].item() for k in ("rec", "kl", "lc", "lap")] + [ce.item(), tot.item()]
    acc = 100.0 * (logits.argmax(1) == torch.tensor(y)).sum().item() / len(y)
    return losses, acc, grads, torch.cat([gc[k].reshape(-1) for k in Pc]), g0


@pytest.mark.parametrize("w_cls", [1.0, 2.0])
def test_train_three_steps_with_head(otopo, dtopo, w_cls):
    """Three steps on the real topology, golden weights, injected key and eps:
    losses (classification and the total included), every VAE gradient, the
    classifier's gradient, and all parameters after the two Adams against the
    oracle.  The head's share of every encoder gradient is at least 5 times the
    comparison's tolerance, so the comparison fails with the term missing."""
    torch.set_num_threads(4)
    w = recipe.golden_weights()
    eng = make_engine(dtopo)
    mlp = make_head(eng, w_cls)
    ref = ref_of(mlp)
    P, Pc = O.make_params(w), dict(ref.named_parameters())
    opt, optc = O.Adam(P), O.Adam(Pc, lr=MLP_LR)
    meshes = recipe.normalized_meshes(12)
    data = torch.from_numpy(meshes).to(DEV)
    table = torch.tensor(LABELS * 3, dtype=torch.int32, device=DEV)
    for step in range(3):
        key = recipe.train_key_index(step)
        eps = torch.from_numpy(recipe.train_eps(step))
        x16 = torch.from_numpy(O.swap_features(meshes[4 * step:4 * step + 4], otopo.region_features, key))
        losses, acc, grads, gcls, g0 = oracle_head_step(P, opt, Pc, optc, ref, x16, otopo, key, eps.numpy(), LABELS,
                                                        w_cls, [0, 5, 10, 15])
        b = eng.inject(eng.buffers(16), key, eps)
        b.batch_idx.copy_(torch.arange(4 * step, 4 * step + 4, dtype=torch.int32))
        b.class_idx = table
        ops.swap_features(data, b.batch_idx, dtopo.region_mask, b.key, 4, out=b.x)
        eng.cls_acc.zero_()
        eng.train_step_on(b)
        torch.cuda.synchronize()
        got, ca = b.losses.cpu().numpy().astype(np.float64), eng.cls_acc.cpu().numpy().astype(np.float64)
        assert ca[2] == 1.0 and int(mlp.step.item()) == step + 1
        np.testing.assert_allclose(list(got[:4]) + [ca[0], got[4] + w_cls * ca[0]], losses, rtol=1e-4)
        assert ca[1] == acc
        hip = {k: v.cpu() for k, v in eng.grads().items()}
        ratios = {}
        for name in w:
            close(hip[name], grads[name], 1e-4, f"step {step} grad {name}")
            if name.startswith("en_layers."):
                tol = 1e-4 * (1.0 + grads[name].abs().max().item())
                ratios[name] = (grads[name] - g0[name]).abs().max().item() / tol
        print(f"w_cls {w_cls} step {step}: head share / tolerance {min(ratios.values()):.1f} "
              f"({min(ratios, key=ratios.get)}) .. {max(ratios.values()):.1f}")
        assert min(ratios.values()) >= 5.0, ratios
        close(eng.head.grad, gcls, 1e-4, f"step {step} classifier grad")
        sd = eng.state_dict()
        for name in w:
            close(sd[name], P[name].detach(), 2e-5, f"step {step} param {name}")
        close(mlp.flat, torch.cat([p.detach().reshape(-1) for p in Pc.values()]), 2e-5, f"step {step} classifier")


def test_step_without_swap_with_head(otopo, dtopo):
    """``swap_features: False``, bs 3: the head reads the 3 consecutive rows;
    one step through TrainStep against the oracle's un-swapped step."""
    torch.set_num_threads(4)
    w, w_cls, y = recipe.golden_weights(), 1.0, [0, 2, 1]
    eng = make_engine(dtopo, bs=3, swap=False)
    mlp = make_head(eng, w_cls)
    ref = ref_of(mlp)
    meshes = recipe.normalized_meshes(12)
    labels = np.arange(12) % 3
    data = E.ResidentData(torch.from_numpy(meshes).to(DEV), bs=3, shuffle=True, class_idx=labels)
    ts = TrainStep(eng, data)
    ts.step()
    torch.cuda.synchronize()
    picked = ts.b.batch_idx.cpu().numpy()
    y = labels[picked].tolist()
    P, Pc = O.make_params(w), dict(ref.named_parameters())
    losses, acc, grads, gcls, _ = oracle_head_step(P, O.Adam(P), Pc, O.Adam(Pc, lr=MLP_LR), ref,
                                                   torch.from_numpy(meshes[picked]), otopo, None,
                                                   ts.b.eps.cpu().numpy(), y, w_cls, [0, 1, 2], want_zero=False)
    got, ca = ts.b.losses.cpu().numpy().astype(np.float64), eng.cls_acc.cpu().numpy().astype(np.float64)
    assert got[2] == 0.0 and abs(ca[1] - acc) <= 1e-5  # the same count of correct rows (100 / 3 is not an fp32 number)
    np.testing.assert_allclose(list(got[:4]) + [ca[0], got[4] + w_cls * ca[0]], losses, rtol=1e-4, atol=1e-7)
    hip = {k: v.cpu() for k, v in eng.grads().items()}
    for name in w:
        close(hip[name], grads[name], 1e-4, f"grad {name}")
    close(eng.head.grad, gcls, 1e-4, "classifier grad")
    sd = eng.state_dict()
    for name in w:
        close(sd[name], P[name].detach(), 2e-5, f"param {name}")
    close(mlp.flat, torch.cat([p.detach().reshape(-1) for p in Pc.values()]), 2e-5, "classifier")


# ---------------------------------------------------------------- graphs
def _runner(dtopo, precision):
    eng = make_engine(dtopo, precision=precision)
    mlp = make_head(eng, 1.0, hidden=(64, 32))
    data = E.ResidentData(torch.from_numpy(recipe.normalized_meshes(12)).to(DEV), bs=4, shuffle=True,
                          class_idx=np.arange(12) % 3)
    return eng, mlp, TrainStep(eng, data)


def _state(eng, mlp):
    torch.cuda.synchronize()
    return {"vae": eng.params.data.clone(), "cls": mlp.flat.clone(), "cls_m": mlp.exp_avg.clone(),
            "cls_acc": eng.cls_acc.clone(), "loss_acc": eng.loss_acc.clone(), "t": mlp.step.clone()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_with_head(dtopo, precision):
    """5 eager steps == capture() + 4 replays == capture() + run(4) through the
    multi-step graph (fp32): VAE and classifier parameters, the classifier's
    moments and step, and both accumulators, bit for bit."""
    eng, mlp, ts = _runner(dtopo, precision)
    for _ in range(5):
        ts.step()
    want = _state(eng, mlp)
    assert want["cls_acc"][2].item() == 5.0 and want["t"].item() == 5
    assert not torch.equal(want["cls"], _runner(dtopo, precision)[1].flat)  # the classifier did train
    eng, mlp, ts = _runner(dtopo, precision)
    ts.capture()
    assert ts.captured and ts.one_graph
    for _ in range(4):
        ts.step()
    got = _state(eng, mlp)
    for k in want:
        assert torch.equal(want[k], got[k]), f"replay: {k}"
    if precision == "fp32":
        eng, mlp, ts = _runner(dtopo, precision)
        ts.steps_per_graph = 2
        ts.capture()
        ts.run(4)
        assert ts.graph_multi is not None
        got = _state(eng, mlp)
        for k in want:
            assert torch.equal(want[k], got[k]), f"multi-step graph: {k}"


def test_gradient_buffer_is_opt_in_and_labels_update_in_place(dtopo):
    """Without ``keep_grad`` a single-GPU step leaves ``head.grad`` alone (the
    Adam launch stores no gradient) and trains the same bits.  New class
    indices are copied into the table a recorded step already reads: the
    replayed step sees them."""
    eng, mlp, ts = _runner(dtopo, "fp32")
    for _ in range(2):
        ts.step()
    want = _state(eng, mlp)
    assert eng.head.keep_grad and eng.head.grad.abs().max().item() > 0
    eng, mlp, ts = _runner(dtopo, "fp32")
    eng.head.keep_grad = False
    ts.capture()
    ts.step()
    got = _state(eng, mlp)
    assert torch.all(eng.head.grad == 0)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    table = ts.data.class_idx
    ts.data.set_class_idx((np.arange(12) + 1) % 3)
    assert ts.data.class_idx is table and table.cpu().tolist() == ((np.arange(12) + 1) % 3).tolist()
    # the same third step eagerly, from the same state, with the new labels
    eng2, mlp2, ts2 = _runner(dtopo, "fp32")
    ts2.step(), ts2.step()
    ts2.data.set_class_idx((np.arange(12) + 1) % 3)
    ts2.step()
    ts.step()  # a replay
    a, b = _state(eng, mlp), _state(eng2, mlp2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # ... and the labels matter: with the old ones the step differs
    eng3, mlp3, ts3 = _runner(dtopo, "fp32")
    for _ in range(3):
        ts3.step()
    assert not torch.equal(_state(eng3, mlp3)["cls"], a["cls"])


def test_no_head_no_change(dtopo):
    """Without a head the step issues no head launch: the launch sequence of a
    step is the same before a head was attached and after it was detached, and
    has exactly two launches fewer than with it."""
    from craniofacialsd_vae_amd import _abi
    eng, mlp, ts = _runner(dtopo, "fp32")
    eng.attach_classifier_head(None, None, 0.0)
    ts.step()
    with _abi.trace_launches() as plain:
        ts.step()
    eng.attach_classifier_head(mlp, torch.tensor(CLASS_W), 1.0)
    with _abi.trace_launches() as with_head:
        ts.step()
    torch.cuda.synchronize()
    names = [r[0] for r in plain]
    assert "cfsd_mlp_head_step" not in names
    assert [r[0] for r in with_head if r[0] != "cfsd_mlp_head_step"] == names
    assert [r[0] for r in with_head].count("cfsd_mlp_head_step") == 1  # (one call: two launches)


# ---------------------------------------------------------------- driver
CONFIG = {
    "optimization": {"epochs": 2, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4, 4, 4]},
              "spirals": {"length": [9, 9, 9, 9], "dilation": [1, 1, 1, 1]}, "in_channels": 3,
              "out_channels": [32, 32, 32, 64], "latent_size": 75, "pre_z_sigmoid": False},
    "classifier": {"main_model_type": "qda", "mlp_training_type": "end2end", "mlp_hidden_features": [32, 16],
                   "mlp_lr": 1e-3, "mlp_epochs": 2, "mlp_loss_weight": 0.5},
    "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
}


@pytest.mark.filterwarnings("ignore:.*not full rank")
def test_driver_trains_end2end_and_resumes(tmp_path, topo_npz):
    """The demo workspace trained for 2 epochs with ``mlp_training_type:
    end2end`` (before the feature: NotImplementedError from the manager)."""
    from craniofacialsd_vae_amd import data as D
    from craniofacialsd_vae_amd import manager as M
    from craniofacialsd_vae_amd import precompute
    from craniofacialsd_vae_amd import train as T
    d = tmp_path
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
    # a split with every class in every part (the i % 100 rule over sorted names puts class a into test and
    # validation only: its weight would be 0 and a validation batch of it alone has no weighted mean)
    names = sorted(os.listdir(d / "meshes"))
    with open(d / "pre" / "data_split.json", "w") as f:
        json.dump({"train": [n for i, n in enumerate(names) if i % 7 > 1],
                   "test": [n for i, n in enumerate(names) if i % 7 == 0],
                   "val": [n for i, n in enumerate(names) if i % 7 == 1]}, f)
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": 89.11,
                             "swap_features": True, "stratified_split": False})
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    man, history = T.main(["--config", str(d / "config.yaml"), "--id", "e2e", "--output_path", str(d / "runs")])
    od = d / "runs" / "outputs" / "e2e"
    op, w_cls = cfg["optimization"], cfg["classifier"]["mlp_loss_weight"]
    assert len(history) == 2
    for h in history:
        for phase in ("train", "validation"):
            r = h[phase]
            assert np.isfinite(r["classification"]) and r["classification"] > 0
            assert 0 <= r["classification_acc"] <= 100
            parts = (r["reconstruction"] + op["kl_weight"] * r["kl"]
                     + op["latent_consistency_weight"] * r["latent_consistency"]
                     + op["laplacian_weight"] * r["laplacian"] + w_cls * r["classification"])
            assert abs(r["tot"] - parts) <= 1e-5 * r["tot"], (phase, r)
    files = sorted(os.listdir(od / "checkpoints"))
    assert {"mlp_classifier.pt", "model_00000001.pt", "model_00000002.pt", "optimizer.pt"} <= set(files)
    logs = [json.loads(ln) for ln in open(od / "logs" / "scalars.jsonl")]
    assert {(x["tag"], x["step"]) for x in logs} >= {(f"{ph}/classification{s}", e) for ph in ("train", "validation")
                                                     for s in ("", "_acc") for e in (1, 2)}
    assert not any("class_loss" in x["tag"] for x in logs)  # no MLP epochs after the VAE (model_manager.py:457)
    saved = torch.load(od / "checkpoints" / "mlp_classifier.pt", weights_only=True)["model"]
    ref = RefMLP([75, 32, 16, 4])
    ref.load_state_dict(saved)  # the reference's format
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in ref.parameters()]), man.classifier_mlp.flat.cpu())
    untrained = C.MLPClassifier(75, [32, 16], 4, device=DEV, seed=0, lr=1e-3)
    assert not torch.equal(untrained.flat, man.classifier_mlp.flat)
    # the classifier stage leaves the MLP alone and reports three accuracies
    tr, va, te, norm = D.load_mesh_dataset(cfg["data"], 4, DEV)
    before = man.classifier_mlp.flat.clone()
    acc = man.train_and_validate_classifiers(tr, va, None, str(tmp_path))
    assert torch.equal(before, man.classifier_mlp.flat)
    assert sorted(acc) == ["lda", "mlp", "qda"] and all(0 <= acc[k] <= 100 for k in acc)
    assert json.load(open(od / "classifiers.json"))["validation_accuracy"] == acc
    # a resumed run's next epoch equals the uninterrupted one
    fresh = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"])
    with pytest.raises(RuntimeError, match="set_class_conversions_and_weights"):
        fresh.run_epoch(tr, train=True)
    fresh.set_class_conversions_and_weights(C.count_labels(tr.labels))
    assert fresh.resume(str(od / "checkpoints")) == 2
    assert torch.equal(fresh.classifier_mlp.flat, man.classifier_mlp.flat)
    tr2 = D.load_mesh_dataset(cfg["data"], 4, DEV)[0]
    third, third_resumed = man.run_epoch(tr, train=True), fresh.run_epoch(tr2, train=True)
    assert third == third_resumed
    assert torch.equal(fresh.engine.params.data, man.engine.params.data)
    assert torch.equal(fresh.classifier_mlp.flat, man.classifier_mlp.flat)
    assert torch.equal(fresh.classifier_mlp.exp_avg_sq, man.classifier_mlp.exp_avg_sq)


# ---------------------------------------------------------------- data parallel
DP_WORKER = r'''
import json, os, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np, torch, torch.distributed as dist
import cfsd_loader, recipe
cfsd_loader.load()
from craniofacialsd_vae_amd import classify as C, engine as E, dist as D, topology
from craniofacialsd_vae_amd.step import TrainStep
world, rank, _ = D.init_from_env(backend="gloo")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
T = topology.DeviceTopology.from_npz(recipe.load_topology(), device=dev)
w = {k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()}
meshes = torch.from_numpy(recipe.normalized_meshes(12)).to(dev)
labels = np.arange(12) % 3

def make(r, seed=3):
    eng = E.SDVAEEngine(T, E.ModelSpec(), seed=1234 + r, device=dev)
    eng.load_state_dict(w)
    mlp = C.MLPClassifier(75, [64, 32], 3, device=dev, seed=seed, lr=1e-3)
    eng.attach_classifier_head(mlp, torch.tensor([0.2, 0.5, 0.3]), 1.0, keep_grad=True)
    lo, hi = D.shard_range(12, r, world)
    data = E.ResidentData(meshes, bs=4, rows=torch.arange(lo, hi), shuffle=True, class_idx=labels)
    return eng, mlp, data

def gather_equal(t):
    gs = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(gs, t.contiguous())
    return all(torch.equal(gs[0], x) for x in gs)

eng, mlp, data = make(rank, seed=3 + rank)   # rank 1's classifier starts elsewhere: the broadcast fixes it
D.broadcast_parameters(mlp.flat, 0)
ts = TrainStep(eng, data, D.GradientAverager(world))
ts.capture()
torch.cuda.synchronize()
g1 = eng.head.grad.cpu().clone()
ts.step(); ts.step()
torch.cuda.synchronize()
res = {"vae_equal": gather_equal(eng.params.data.cpu()), "cls_equal": gather_equal(mlp.flat.cpu()),
       "cls_step": int(mlp.step.item()), "cls_steps_counted": float(eng.cls_acc[2].item())}
if rank == 0:
    singles = []
    for r in range(world):
        e1, m1, d1 = make(r)
        TrainStep(e1, d1).step()
        torch.cuda.synchronize()
        singles.append(e1.head.grad.cpu())
    mean = (singles[0].double() + singles[1].double()) * 0.5
    res["grad_err"] = float((g1.double() - mean).abs().max())
    res["grad_tol"] = 1e-5 * (1.0 + float(mean.abs().max()))
    res["groups_differ"] = not torch.equal(singles[0], singles[1])
    res["trained"] = not torch.equal(mlp.flat.cpu(), make(0)[1].flat.cpu())
    with open(OUT, "w") as f:
        json.dump(res, f)
dist.barrier()
dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_dp2_trainstep_with_head(tmp_path):
    """2 ranks, graph-replayed TrainStep with a head, through the launcher of
    test_gpu_dist.py: two gloo ranks sharing the one test GPU, so it needs no
    second GPU and is never skipped (gloo cannot be captured: this is the
    three-graph structure with host-issued collectives).  After 3 steps the VAE and the classifier are identical on
    both ranks; the classifier's first-step gradient is the mean of the two
    single-rank gradients of the same batches."""
    wfile, out = tmp_path / "dp_worker.py", tmp_path / "res.json"
    wfile.write_text(DP_WORKER)
    env = dict(os.environ, CFSD_DIST_BACKEND="gloo", CFSD_SHARE_DEVICE="1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(wfile), ROOT, str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["groups_differ"] and res["trained"], res
    assert res["vae_equal"] and res["cls_equal"] and res["cls_step"] == 3 and res["cls_steps_counted"] == 3.0, res
    assert res["grad_err"] <= res["grad_tol"], res


RCCL_WORKER = r'''
import json, os, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np, torch, torch.distributed as dist
import cfsd_loader, recipe
cfsd_loader.load()
from craniofacialsd_vae_amd import classify as C, engine as E, dist as D, topology
from craniofacialsd_vae_amd.step import TrainStep
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)
T = topology.DeviceTopology.from_npz(recipe.load_topology(), device=dev)
w = {k: torch.from_numpy(v) for k, v in recipe.golden_weights().items()}
meshes = torch.from_numpy(recipe.normalized_meshes(12)).to(dev)
runs = {}
for mode in ("single", "rccl_one_graph"):
    eng = E.SDVAEEngine(T, E.ModelSpec(), seed=7, device=dev)
    eng.load_state_dict(w)
    mlp = C.MLPClassifier(75, [64, 32], 3, device=dev, seed=3, lr=1e-3)
    eng.attach_classifier_head(mlp, torch.tensor([0.2, 0.5, 0.3]), 1.0, keep_grad=True)
    data = E.ResidentData(meshes, bs=4, shuffle=True, class_idx=np.arange(12) % 3)
    ts = TrainStep(eng, data, None if mode == "single" else D.GradientAverager(1, always=True))
    ts.steps_per_graph = 2
    ts.capture()      # step 1, eager
    ts.step()         # step 2, one replay
    ts.run(4)         # steps 3-6, the two-step graph twice
    torch.cuda.synchronize()
    runs[mode] = {"state": [t.detach().cpu().clone() for t in (eng.params.data, eng.params.exp_avg_sq, mlp.flat,
                                                                mlp.exp_avg, mlp.exp_avg_sq, mlp.step, eng.cls_acc,
                                                                eng.loss_acc, eng.head.grad)],
                  "one_graph": ts.one_graph, "dp": ts.avg is not None, "multi": ts.graph_multi is not None,
                  "fallback": ts.fallback}
names = ["vae", "vae_v", "cls", "cls_m", "cls_v", "cls_t", "cls_acc", "loss_acc", "cls_grad"]
a, s = runs["rccl_one_graph"], runs["single"]
res = {"one_graph": a["one_graph"], "dp": a["dp"], "multi": a["multi"], "fallback": a["fallback"],
       "differs": [n for n, x, y in zip(names, a["state"], s["state"]) if not torch.equal(x, y)],
       "cls_t": int(s["state"][5].item()), "cls_steps": float(s["state"][6][2].item())}
with open(OUT, "w") as f:
    json.dump(res, f)
dist.destroy_process_group()
'''


def test_rccl_world1_one_graph_with_head(tmp_path):
    """A one-rank RCCL group runs the data-parallel structure on one GPU: the
    classifier's gradient bucket is all-reduced INSIDE the captured step graph
    and the multi-step graph, and its Adam is the separate scaled launch.
    After 6 steps everything equals the single-process step bit for bit (a sum
    over one rank and a scale by 1 change nothing)."""
    wfile, out = tmp_path / "worker.py", tmp_path / "res.json"
    wfile.write_text(RCCL_WORKER)
    cmd = [sys.executable, "-u", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(wfile), ROOT, str(out)]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["dp"] and res["one_graph"] and res["multi"] and res["fallback"] is None, res
    assert res["cls_t"] == 6 and res["cls_steps"] == 6.0, res
    assert res["differs"] == [], res
