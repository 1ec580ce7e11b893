"""The per-batch backward plan (``bwd_plan.py``): the launch sequence of a
train step is pinned per configuration (``tests/golden/launch_plans.json``,
written by ``tests/golden/make_launch_plans.py``), every layer's
weight-gradient region covers what its kind asks for, and the general
``Pool(down)`` path (a down-sampling matrix that is no 0/1 selection) trains
in lock-step with the oracle on a small torus (needs an MI355X).
"""
import numpy as np
import pytest
import torch

import cfsd_loader
import make_launch_plans as LP
import synthetic_topology as ST
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import ops  # noqa: E402


@pytest.fixture(scope="module", params=sorted(LP.CONFIGS))
def case(request):
    eng, _ = LP.make_engine(request.param)
    return request.param, eng, LP.record_step(request.param, eng)


@pytest.fixture(scope="module")
def fixture_plans():
    return LP.load_fixture()


def test_launch_sequence_matches_fixture(case, fixture_plans):
    """One eager step issues exactly the recorded launches: entry points,
    order, every int / float argument (workspace byte counts included) and
    the slab geometry of every deferred weight gradient."""
    name, _, got = case
    want = fixture_plans[name]
    assert [g[0] for g in got] == [w[0] for w in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"config {name}, launch {k} ({w[0]})"


def test_plan_regions_cover_their_kind(case):
    """Sizing and dispatch agree: each layer's region of ``b.ws_dw_all`` holds
    at least the workspace query of the kind the plan chose, and no two
    regions overlap."""
    name, eng, _ = case
    b = eng.buffers(LP.CONFIGS[name][4])
    assert set(b.plan) == set(b.ws_dw)
    spans = []
    for key, layer in b.plan.items():
        region = b.ws_dw[key]
        assert region.numel() * 4 >= layer.workspace(layer) == layer.nbytes, (key, layer.kind.__name__)
        lo = region.data_ptr() - b.ws_dw_all.data_ptr()
        assert 0 <= lo and lo + region.numel() * 4 <= b.ws_dw_all.numel() * 4
        spans.append((lo, lo + region.numel() * 4, key))
    spans.sort(key=lambda s: s[:2])
    for (_, end, k0), (start, _, k1) in zip(spans, spans[1:]):
        assert end <= start, f"regions {k0} and {k1} overlap"


def _close(a, b, rel, what):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    err, tol = np.abs(a - b).max(), rel * (1.0 + np.abs(b).max())
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"


@pytest.mark.parametrize("which,select", [pytest.param("all", [False, False, False], id="all"),
                                          pytest.param("mixed", [True, False, True], id="mixed")])
def test_nonselection_step_vs_oracle(which, select):
    """The general Pool(down) path (full-resolution Enblock conv, SpMM down,
    Pool(down)^T SpMM in the backward): three steps in lock-step with the
    oracle on the 288-vertex torus whose down-sampling averages two vertices,
    with test_c4_train_three_steps's checks and tolerances."""
    torch.set_num_threads(1)
    name = {"all": "h", "mixed": "i"}[which]
    eng, dtopo = LP.make_engine(name)
    assert dtopo.enc_select == select and dtopo.n_verts == [288, 144, 72, 36]
    assert not eng.fuse_bottleneck
    T = O.Topology(LP.topology_npz(LP.CONFIGS[name][0]))
    w = LP.body_weights(36)
    P = O.make_params(w)
    opt = O.Adam(P)
    shadow = {k: torch.from_numpy(v.copy()) for k, v in w.items()}
    shadow_opt = O.Adam(shadow)
    meshes = ST.torus_meshes(12, nu=LP.SMALL["nu"], nv=LP.SMALL["nv"], seed=2)
    data = torch.from_numpy(meshes).cuda()
    for step in range(3):
        key = (2 + 4 * step) % 11
        out, grads, x16 = O.train_step(P, opt, meshes[4 * step:4 * step + 4], T, key, None,
                                       w=LP.W_BODY, is_vae=False)
        b = eng.buffers(16)
        b.key.fill_(key)
        b.batch_idx.copy_(torch.arange(4 * step, 4 * step + 4, dtype=torch.int32))
        ops.swap_features(data, b.batch_idx, dtopo.region_mask, b.key, 4, out=b.x)
        eng.train_step_on(b)
        torch.cuda.synchronize()
        assert np.array_equal(b.x.cpu().numpy(), x16.numpy()), f"step {step}: swap differs"
        ref = np.array([out[k].item() for k in ("rec", "kl", "lc", "lap", "tot")])
        got = b.losses.cpu().numpy()
        d = np.abs(b.out.cpu().numpy() - out["out"].detach().numpy()).sum(-1)
        print(f"step {step}: losses {got.tolist()} ref {ref.tolist()} max per-vertex L1 {d.max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-7)
        assert d.max() <= 1e-4, f"step {step}: max per-vertex L1 {d.max():.3e}"
        hip_grads = {k: g.detach().cpu().clone() for k, g in eng.grads().items()}
        for gname, g in hip_grads.items():
            _close(g, grads[gname], 1e-4, f"step {step} grad {gname}")
        # Adam against the restated torch.optim.Adam rule on the device's own gradients
        shadow_opt.step(shadow, hip_grads)
        sd = eng.state_dict()
        for pname in w:
            _close(sd[pname], shadow[pname], 1e-6, f"step {step} adam {pname}")
            assert (sd[pname].cpu() - P[pname].detach()).abs().max() <= 2e-4 * (step + 1) + 1e-6
