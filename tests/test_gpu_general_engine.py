"""The training step on architectures outside the specialised kernels' shape
lists: other spiral lengths (uniform 7 and 12, mixed 7 / 12 with dilation) and
channel widths ([8, 20], [12, 40]), in lock-step with the oracle at the
tolerances of test_c4_body (losses rtol 1e-4, per-vertex L1 <= 1e-4, gradients
rel 1e-4, Adam vs the restated rule 1e-6); the backward plan; graph capture;
and the YAML driver with save / resume.  Before the general-shape kernels the
first step of every engine here raised."""
import os

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe
import synthetic_topology as ST
from oracle import cfsd_oracle as O

pytestmark = pytest.mark.gpu

cfsd_loader.load()
from craniofacialsd_vae_amd import bwd_plan, ops, precompute, topology  # noqa: E402
from craniofacialsd_vae_amd import engine as E  # noqa: E402
from craniofacialsd_vae_amd.step import TrainStep  # noqa: E402

DEV = "cuda"
UNIFORM = {7: ([8, 20], 22), 12: ([12, 40], 33)}  # spiral length -> (out_channels, latent)


@pytest.fixture(scope="module")
def uniform_npz():
    return {S: ST.torus_topology(nu=32, nv=16, factors=(4, 4), seq=S) for S in UNIFORM}


def uniform_weights(S):
    out_ch, latent = UNIFORM[S]
    return recipe.golden_weights(recipe.param_shapes(num_vert=32, out_ch=out_ch, latent=latent, seq=S), seed=4)


def uniform_engine(npz, S, **kw):
    out_ch, latent = UNIFORM[S]
    dtopo = topology.DeviceTopology.from_npz(npz, device=DEV)
    assert dtopo.n_verts == [512, 128, 32] and dtopo.seq == [S, S] and dtopo.n_regions == 11
    eng = E.SDVAEEngine(dtopo, E.ModelSpec(3, out_ch, latent), swap_bs=4, device=DEV, **kw)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in uniform_weights(S).items()})
    return dtopo, eng


def _close(a, b, rel, what):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    err, tol = np.abs(a - b).max(), rel * (1.0 + np.abs(b).max())
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"


def lockstep(eng, dtopo, otopo, weights, meshes, latent, n_steps, n_regions):
    """``n_steps`` train steps of the engine and the oracle side by side (the pattern of
    test_c4_body.test_c4_train_three_steps, with injected VAE noise)."""
    P = O.make_params(weights)
    opt = O.Adam(P)
    shadow = {k: torch.from_numpy(v.copy()) for k, v in weights.items()}
    shadow_opt = O.Adam(shadow)
    data = torch.from_numpy(meshes).to(DEV)
    for step in range(n_steps):
        key = (2 + 4 * step) % n_regions
        eps = np.random.RandomState(100 + step).randn(16, latent).astype(np.float32)
        out, grads, x16 = O.train_step(P, opt, meshes[4 * step:4 * step + 4], otopo, key, eps)
        b = eng.inject(eng.buffers(16), key, torch.from_numpy(eps))
        b.batch_idx.copy_(torch.arange(4 * step, 4 * step + 4, dtype=torch.int32))
        ops.swap_features(data, b.batch_idx, dtopo.region_mask, b.key, 4, out=b.x)
        eng.train_step_on(b)
        torch.cuda.synchronize()
        assert np.array_equal(b.x.cpu().numpy(), x16.numpy()), f"step {step}: swap differs"
        ref = np.array([out[k].item() for k in ("rec", "kl", "lc", "lap", "tot")])
        np.testing.assert_allclose(b.losses.cpu().numpy(), ref, rtol=1e-4, atol=1e-7)
        d = np.abs(b.out.cpu().numpy() - out["out"].detach().numpy()).sum(-1)
        assert d.max() <= 1e-4, f"step {step}: max per-vertex L1 {d.max():.3e}"
        hip_grads = {k: g.detach().cpu().clone() for k, g in eng.grads().items()}
        assert set(hip_grads) == set(grads)
        for name, g in hip_grads.items():
            _close(g, grads[name], 1e-4, f"step {step} grad {name}")
        # Adam: the device update equals the restated rule applied to the device's own gradients
        shadow_opt.step(shadow, hip_grads)
        sd = eng.state_dict()
        for name in weights:
            _close(sd[name], shadow[name], 1e-6, f"step {step} adam {name}")
            assert (sd[name].cpu() - P[name].detach()).abs().max() <= 2e-4 * (step + 1) + 1e-6


@pytest.mark.parametrize("S", sorted(UNIFORM))
def test_uniform_spiral_length_three_steps(uniform_npz, S):
    torch.set_num_threads(4)
    npz = uniform_npz[S]
    dtopo, eng = uniform_engine(npz, S)
    meshes = ST.torus_meshes(12, nu=32, nv=16, seed=2)
    lockstep(eng, dtopo, O.Topology(npz), uniform_weights(S), meshes, UNIFORM[S][1], 3, 11)


def test_mixed_spiral_lengths_one_step():
    """Spiral lengths (7, 12) with dilations (1, 2), built by precompute and loaded by both sides."""
    torch.set_num_threads(4)
    npz = precompute.build_hierarchy(*precompute.torus(32, 16), sampling_factors=(4, 4), seq_lengths=(7, 12),
                                     dilations=(1, 2))
    dtopo, otopo = topology.DeviceTopology.from_npz(npz, device=DEV), O.Topology(npz)
    assert dtopo.seq == [7, 12] and dtopo.n_verts == [512, 128, 32]
    n_reg = dtopo.n_regions
    latent = 2 * n_reg
    spec = E.ModelSpec(3, [8, 20], latent)
    weights = recipe.golden_weights(spec.param_specs(32, dtopo.seq), seed=4)
    weights = {k: weights[k] for k in spec.reference_order(32, dtopo.seq)}
    eng = E.SDVAEEngine(dtopo, spec, swap_bs=4, device=DEV)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    rs = np.random.RandomState(7)
    meshes = (npz["pos_0"][None] + 0.05 * rs.randn(4, 512, 3)).astype(np.float32)
    lockstep(eng, dtopo, otopo, weights, meshes, latent, 1, n_reg)
    b = eng.buffers(16)
    assert all(L.kind is bwd_plan.general for L in b.plan.values())


def test_plan_general_and_specialised(uniform_npz):
    _, eng = uniform_engine(uniform_npz[7], 7)
    b = eng.buffers(16)
    assert len(b.plan) == 5 and all(L.kind is bwd_plan.general for L in b.plan.values())
    assert b.xl == set() and eng.vm_levels(16) == set()
    for fams in (bwd_plan.OUT_KINDS, bwd_plan.DEC_KINDS, bwd_plan.ENC_KINDS):
        assert fams[0][0] is bwd_plan.general  # tried first
    # the default architecture on a spiral-length-9 hierarchy: nothing general, vertex-major levels kept.
    # (1024 / 256 / 64 / 16 / 4 vertices: the smallest torus the edge collapse takes through four
    # levels -- synthetic_hierarchy(16, 16) raises "zero-size array to reduction operation
    # maximum": its last level would be a single vertex, which has no face)
    h = precompute.synthetic_hierarchy(n_major=32, n_minor=32, device=DEV)
    assert h.n_verts == [1024, 256, 64, 16, 4] and h.seq == [9, 9, 9, 9]
    e9 = E.SDVAEEngine(h, E.ModelSpec(3, (32, 32, 32, 64), 75), swap_bs=4, device=DEV, w_lc=0.0)
    b9 = e9.buffers(16)
    assert len(b9.plan) == 9 and not any(L.kind is bwd_plan.general or L.general for L in b9.plan.values())
    assert e9.vm_levels(16) == {0, 1} and b9.xl == {0, 1}
    # bf16 has no general-shape kernels: refused with the layer and its shape
    dtopo = topology.DeviceTopology.from_npz(uniform_npz[7], device=DEV)
    with pytest.raises(ValueError, match=r"en_layers\.0\.conv\.layer \(spiral length 7, 3 -> 8"):
        E.SDVAEEngine(dtopo, E.ModelSpec(3, [8, 20], 22), swap_bs=4, device=DEV, precision="bf16")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("in_ch", [1, 2, 3])
def test_vertex_major_plan_is_the_specialised_one(in_ch, precision):
    """Spiral length 9, widths (32, 32, 32, 64), batch 16: levels 0 and 1 are vertex-major and
    the general kernels batch-major only, so no layer may be ``general`` -- also not the output
    conv 32 -> 1 / 2 and the input conv 1 / 2 -> 32, which the fp32 batch-major forward, dx and
    dW entry points have no instance for (the fused backward and the vertex-major entry points
    do).  Every layer keeps the kind it had before ``general`` existed: the first of the others
    that applies.  bf16 accepts the same architectures."""
    h = precompute.synthetic_hierarchy(n_major=32, n_minor=32, device=DEV)
    eng = E.SDVAEEngine(h, E.ModelSpec(in_ch, (32, 32, 32, 64), 75), swap_bs=4, device=DEV, w_lc=0.0,
                        precision=precision)
    b = eng.buffers(16)
    assert eng.vm_levels(16) == {0, 1} and b.xl == {0, 1} and len(b.plan) == 9
    fams = {"out": bwd_plan.OUT_KINDS, "dec": bwd_plan.DEC_KINDS, "enc": bwd_plan.ENC_KINDS}
    for key, L in b.plan.items():
        fam = fams[key if key == "out" else key[0]]
        before = next(k for k, applies, _ in fam if k is not bwd_plan.general and applies(L, eng))
        assert not L.general and L.kind is before, (key, L.kind.__name__, before.__name__)
        assert L.vm == (L.lv in (0, 1))
    want = bwd_plan.out_flat if in_ch == 3 else bwd_plan.out_x
    assert b.plan["out"].kind is want and b.plan["enc", 0].kind is bwd_plan.weight_x_inv
    assert b.plan["out"].nbytes == ops.spiral_conv_bwd_workspace(16, 1024, 1024, 9, 32, in_ch) > 0


@pytest.mark.parametrize("structure", ["one-step", "multi-step"])
def test_captured_step_equals_eager(uniform_npz, structure):
    """The S = 7 step recorded by TrainStep and replayed, against the same steps run eagerly."""
    meshes = torch.from_numpy(ST.torus_meshes(12, nu=32, nv=16, seed=3)).to(DEV)
    runs = []
    for captured in (False, True):
        _, eng = uniform_engine(uniform_npz[7], 7, seed=5)
        ts = TrainStep(eng, E.ResidentData(meshes, 4))
        if not captured:
            for _ in range(3):
                ts.step()
        else:
            ts.steps_per_graph = 2 if structure == "multi-step" else 1
            ts.capture()               # one eager step, then the recording
            assert ts.one_graph and ts.captured
            ts.run(2)                  # multi-step: one replay of the two-step graph; else two replays
            assert (ts.graph_multi is not None) == (structure == "multi-step")
        torch.cuda.synchronize()
        P = eng.params
        runs.append([t.clone() for t in (P.data, P.grad, P.exp_avg, P.exp_avg_sq, eng.loss_acc, ts.b.out)])
        assert int(P.step.item()) == 3 and torch.isfinite(eng.loss_acc).all()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


CONFIG = {
    "optimization": {"epochs": 1, "batch_size": 4, "lr": 1e-4, "weight_decay": 0, "laplacian_weight": 0.1,
                     "kl_weight": 1e-4, "latent_consistency_weight": 0.5, "latent_consistency_eta1": 0.5,
                     "latent_consistency_eta2": 0.5},
    "model": {"sampling": {"type": "basic", "sampling_factors": [4, 4]},
              "spirals": {"length": [7, 12], "dilation": [1, 2]}, "in_channels": 3,
              "out_channels": [8, 20], "latent_size": 30, "pre_z_sigmoid": False},
    "logging_frequency": {"tb_renderings": 50, "save_weights": 1},
}


def test_driver_trains_saves_and_resumes(tmp_path):
    """A ModelManager from a config whose spirals.length, spirals.dilation and out_channels are
    not the defaults (the hierarchy is precomputed from the template): one epoch, a checkpoint,
    and a resumed manager whose next epoch equals the uninterrupted one."""
    from craniofacialsd_vae_amd import data as D
    from craniofacialsd_vae_amd import manager as M
    d = tmp_path
    pos, faces, colors = precompute.torus(32, 16)
    precompute.write_ply(str(d / "template.ply"), pos, faces, colors)
    (d / "meshes").mkdir()
    rs = np.random.RandomState(3)
    for i in range(24):
        v = (pos + rs.normal(0, 0.02, pos.shape)).astype(np.float32)
        with open(d / "meshes" / f"{'nacm'[i % 4]}_{i:03d}.obj", "w") as f:
            for p in v:
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
    cfg = dict(CONFIG, data={"template_path": str(d / "template.ply"), "precomputed_path": str(d / "pre"),
                             "dataset_path": str(d / "meshes"), "normalize_data": True, "to_mm_constant": 1.0,
                             "swap_features": True, "stratified_split": False})
    man = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"])
    assert man.topology.seq == [7, 12] and os.path.exists(d / "pre" / "topology.npz")
    assert all(L.kind is bwd_plan.general for L in man.engine.buffers(16).plan.values())
    tr = D.load_mesh_dataset(cfg["data"], 4, DEV)[0]
    first = man.run_epoch(tr, train=True)
    assert all(np.isfinite(v) for v in first.values()) and first["reconstruction"] > 0
    ckpt = d / "checkpoints"
    ckpt.mkdir()
    man.save_weights(str(ckpt), 0)
    sd = torch.load(ckpt / "model_00000001.pt", weights_only=True)["model"]
    assert tuple(sd["en_layers.0.conv.layer.weight"].shape) == (8, 7 * 3)
    assert tuple(sd["de_layers.1.conv.layer.weight"].shape) == (20, 12 * 20)
    assert tuple(sd["de_layers.3.layer.weight"].shape) == (3, 7 * 8)
    fresh = M.ModelManager(cfg, device=DEV, precomputed_storage_path=cfg["data"]["precomputed_path"])
    assert fresh.resume(str(ckpt)) == 1
    assert torch.equal(fresh.engine.params.data, man.engine.params.data)
    tr2 = D.load_mesh_dataset(cfg["data"], 4, DEV)[0]
    second, second_resumed = man.run_epoch(tr, train=True), fresh.run_epoch(tr2, train=True)
    assert second == second_resumed
    assert torch.equal(fresh.engine.params.data, man.engine.params.data)
    # an architecture the kernels cannot run is refused before the precompute, by its YAML key
    bad = dict(cfg, model=dict(cfg["model"], out_channels=[6, 20]),
               data=dict(cfg["data"], precomputed_path=str(d / "pre_bad")))
    with pytest.raises(ValueError, match=r"model\.out_channels"):
        M.ModelManager(bad, device=DEV, precomputed_storage_path=str(d / "pre_bad"))
    assert not os.path.exists(d / "pre_bad")
