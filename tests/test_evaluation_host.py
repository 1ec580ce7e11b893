"""CPU tests of the evaluation harness's host side (``evaluation.py``): the
restated scikit-learn reports against recorded scikit-learn output, the latent
schedules against ``torch.linspace`` / ``torch.randn``, the animated PNG writer
chunk by chunk, the refusals of the two C entries of ``csrc/evaluate.hip``
(before any HIP call) and of ``topology.RegionCSR``.  No kernel is launched."""
import ctypes
import json
import os
import struct
import types
import zlib

import numpy as np
import pytest
import torch

import cfsd_loader
import recipe

cfsd_loader.load()
from craniofacialsd_vae_amd import _abi, evaluation, ops, rendering, topology  # noqa: E402

LATENT = 6


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libcfsd.so not built (run __graft_entry__.build())")
    return _abi.load()


@pytest.fixture(scope="module")
def sk():
    with open(os.path.join(recipe.HERE, "evaluate_sklearn.json")) as f:
        return json.load(f)["cases"]


# ------------------------------------------------------------------ reports
def _flat(report):
    out = {}
    for k, v in report.items():
        for kk, vv in (v.items() if isinstance(v, dict) else [("", v)]):
            out[(k, kk)] = vv
    return out


SK_CASES = ["four_classes", "predicted_but_absent", "never_predicted", "single_class", "integers", "all_wrong"]


@pytest.mark.parametrize("name", SK_CASES)
def test_reports_match_sklearn(sk, name):
    """Float64 throughout: every figure within 1e-12 of scikit-learn 1.7.2's,
    the keys and their order the same, supports equal as integers."""
    c = sk[name]
    got = evaluation.classification_report(c["y_true"], c["y_pred"])
    assert list(got) == list(c["report"])
    g, r = _flat(got), _flat(c["report"])
    assert list(g) == list(r)
    for key in r:
        if key[1] == "support":
            assert isinstance(g[key], int) and g[key] == r[key], key
        else:
            assert isinstance(g[key], float) and abs(g[key] - r[key]) <= 1e-12, key
    json.dumps(got)  # plain Python numbers
    cm = evaluation.confusion_matrix(c["y_true"], c["y_pred"], normalize="true")
    assert cm.dtype == np.float64 and np.abs(cm - np.asarray(c["confusion_true"])).max() <= 1e-12
    counts = evaluation.confusion_matrix(np.asarray(c["y_true"]), np.asarray(c["y_pred"]))
    assert np.array_equal(counts, np.asarray(c["confusion_counts"]))
    assert evaluation._labels_of(c["y_true"], c["y_pred"]) == c["labels"]


def test_report_edge_cases(sk):
    """The cases the recorded vectors were chosen for, read off the results."""
    absent = evaluation.classification_report(*[sk["predicted_but_absent"][k] for k in ("y_true", "y_pred")])
    assert absent["a"] == {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 0}
    cm = evaluation.confusion_matrix(*[sk["predicted_but_absent"][k] for k in ("y_true", "y_pred")], normalize="true")
    assert not cm[0].any() and np.allclose(cm[1:].sum(1), 1.0)  # the row without support is zeros
    never = evaluation.classification_report(*[sk["never_predicted"][k] for k in ("y_true", "y_pred")])
    assert never["a"]["precision"] == 0.0 and never["a"]["recall"] == 0.0 and never["a"]["support"] == 3
    single = evaluation.classification_report(list("nnnnn"), list("nnnnn"))
    assert list(single) == ["n", "accuracy", "macro avg", "weighted avg"] and single["accuracy"] == 1.0
    with pytest.raises(ValueError):
        evaluation.classification_report(["a"], ["a", "c"])
    with pytest.raises(ValueError):
        evaluation.confusion_matrix(["a"], ["a"], normalize="pred")


# ------------------------------------------------------------------ latents
def _tester(tmp_path, is_vae, stats=None):
    """A Tester over a stand-in manager: nothing here touches the device."""
    g = torch.Generator().manual_seed(4)
    if stats is None:
        lo = torch.randn(LATENT, generator=g) - 2
        stats = {"means": torch.randn(LATENT, generator=g), "stds": torch.rand(LATENT, generator=g),
                 "mins": lo, "maxs": lo + torch.rand(LATENT, generator=g) * 4 + 0.1}
    manager = types.SimpleNamespace(net=types.SimpleNamespace(eval=lambda: None), device=torch.device("cpu"),
                                    is_vae=is_vae, bs=2, latent_regions={"r0": [0, 3], "r1": [3, 6]})
    config = {"data": {"normalize_data": False, "swap_features": True}, "model": {"latent_size": LATENT}}
    return evaluation.Tester(manager, None, None, None, str(tmp_path), config, latent_stats=stats), stats


def test_vector_linspace():
    a, b = torch.tensor([[0.1, -2.0, 3.5]]), torch.tensor([[1.7, 2.0, 3.5]])
    for steps in (1, 2, 7):
        got = evaluation.vector_linspace(a, b, steps)
        assert got.shape == (steps, 3)
        for j in range(3):
            assert torch.equal(got[:, j], torch.linspace(a[0, j].item(), b[0, j].item(), steps))
    assert evaluation.Tester.vector_linspace is evaluation.vector_linspace


@pytest.mark.parametrize("is_vae,use_z_stats,mult", [(True, False, 1), (True, False, 2), (True, True, 1.5),
                                                     (False, False, 0.5), (False, True, 1)])
def test_traversal_latents(tmp_path, is_vae, use_z_stats, mult):
    """Row i: the means everywhere, column i = torch.linspace(min_i, max_i),
    bit for bit.  Only a VAE without statistics walks [-3 m, 3 m] around 0."""
    t, stats = _tester(tmp_path, is_vae)
    for n_steps in (10, 3):
        z = t.traversal_latents(mult, use_z_stats, n_steps)
        assert z.shape == (LATENT, n_steps, LATENT) and z.dtype == torch.float32
        if is_vae and not use_z_stats:
            means, lo, hi = torch.zeros(LATENT), -3 * mult * torch.ones(LATENT), 3 * mult * torch.ones(LATENT)
        else:
            means, lo, hi = stats["means"], stats["mins"] * mult, stats["maxs"] * mult
        for i in range(LATENT):
            assert torch.equal(z[i, :, i], torch.linspace(lo[i], hi[i], n_steps))
            others = [j for j in range(LATENT) if j != i]
            assert torch.equal(z[i][:, others], means[others].expand(n_steps, -1))


def test_random_latent(tmp_path):
    vae, _ = _tester(tmp_path, True)
    a = vae.random_latent(5, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, torch.randn([5, LATENT], generator=torch.Generator().manual_seed(9)))
    assert torch.equal(a, vae.random_latent(5, generator=torch.Generator().manual_seed(9)))
    assert not torch.equal(a, vae.random_latent(5, generator=torch.Generator().manual_seed(10)))
    ae, stats = _tester(tmp_path, False)
    for m in (1, 2.5):
        z = ae.random_latent(400, m, generator=torch.Generator().manual_seed(1))
        assert z.shape == (400, LATENT)
        assert torch.equal(z, ae.random_latent(400, m, generator=torch.Generator().manual_seed(1)))
        lo, hi = stats["mins"] * m, stats["maxs"] * m
        assert bool((z >= torch.minimum(lo, hi)).all()) and bool((z <= torch.maximum(lo, hi)).all())
        assert z.std(0).min() > 0


def test_tester_reads_and_writes_z_stats(tmp_path):
    """z_stats.pt in the output folder is read back (tensors only)."""
    stats = {k: torch.arange(LATENT, dtype=torch.float32) + i for i, k in enumerate(("means", "stds", "mins", "maxs"))}
    torch.save(stats, tmp_path / "z_stats.pt")
    manager = types.SimpleNamespace(net=types.SimpleNamespace(eval=lambda: None), device=torch.device("cpu"),
                                    is_vae=True, bs=2, latent_regions={})
    config = {"data": {"normalize_data": False}, "model": {"latent_size": LATENT}}
    t = evaluation.Tester(manager, None, None, None, str(tmp_path), config)
    assert all(torch.equal(t.latent_stats[k], stats[k]) for k in stats)
    assert not t.has_classifiers
    with pytest.raises(RuntimeError):
        t.test_classifiers()
    with pytest.raises(NotImplementedError):
        t.embeddings(mode="tsne")


# ------------------------------------------------------------------ APNG
def parse_apng(path):
    """The chunks of a PNG file, every CRC checked."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(raw)
    return chunks


def check_apng(path, n_frames, fps=None):
    """Structure of an animated PNG; returns its frames as ``[N, H, W, 3]`` uint8."""
    chunks = parse_apng(path)
    tags = [t for t, _ in chunks]
    assert tags[:2] == [b"IHDR", b"acTL"] and tags[-1] == b"IEND" and chunks[-1][1] == b""
    assert tags[2:-1] == [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n_frames - 1)
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    assert struct.unpack(">II", chunks[1][1]) == (n_frames, 0)  # num_frames, num_plays = 0: for ever
    seq, frames = 0, []
    for tag, body in chunks[2:-1]:
        if tag == b"fcTL":
            s, fw, fh, x0, y0, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (s, fw, fh, x0, y0, dispose, blend) == (seq, w, h, 0, 0, 0, 0)
            if fps is not None:
                assert num * fps == den  # delay = 1 / fps
            seq += 1
            continue
        if tag == b"fdAT":
            assert struct.unpack(">I", body[:4])[0] == seq
            seq += 1
            body = body[4:]
        rows = np.frombuffer(zlib.decompress(body), np.uint8).reshape(h, 1 + 3 * w)
        assert not rows[:, 0].any()
        frames.append(rows[:, 1:].reshape(h, w, 3))
    assert seq == 2 * n_frames - 1
    return np.stack(frames)


@pytest.mark.parametrize("n_frames", [1, 3])
def test_save_apng_round_trip(tmp_path, n_frames):
    rs = np.random.RandomState(n_frames)
    frames = torch.from_numpy(rs.rand(n_frames, 3, 5, 9).astype(np.float32) * 1.4 - 0.2)  # clamped by to_uint8
    path = rendering.save_apng(str(tmp_path / "a.apng"), frames, fps=4)
    back = check_apng(path, n_frames, fps=4)
    for k in range(n_frames):
        np.testing.assert_array_equal(back[k], rendering.to_uint8(frames[k]))
    u8 = torch.from_numpy(rs.randint(0, 256, (n_frames, 3, 4, 6)).astype(np.uint8))
    back = check_apng(rendering.save_apng(str(tmp_path / "b.apng"), u8, fps=1), n_frames, fps=1)
    np.testing.assert_array_equal(back, u8.numpy().transpose(0, 2, 3, 1))
    for bad in (torch.zeros(3, 4, 4), torch.zeros(2, 1, 4, 4), torch.zeros(0, 3, 4, 4)):
        with pytest.raises(ValueError):
            rendering.save_apng(str(tmp_path / "c.apng"), bad, fps=4)
    with pytest.raises(ValueError):
        rendering.save_apng(str(tmp_path / "c.apng"), u8, fps=0)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.size == (9, 5) and getattr(im, "n_frames", 1) == n_frames


# ------------------------------------------------------------------ entry points
def test_evaluate_entry_points_validate_before_any_hip_call(lib):
    p = ctypes.c_void_p(256)
    assert lib.cfsd_version() >> 16 == 4 and (lib.cfsd_version() & 0xffff) >= 17
    err = lib.cfsd_last_error_string

    def group(frames=p, mean=p, std=p, out=p, groups=2, n=3, nv=5):
        return lib.cfsd_group_vertex_errors(frames, mean, std, out, groups, n, nv, 1.0, None)

    for kw in ({"frames": None}, {"out": None}):
        assert group(**kw) == -1 and b"null" in err()
    for kw in ({"mean": None}, {"std": None}):
        assert group(**kw) == -1 and b"go together" in err()
    for kw in ({"groups": 0}, {"n": 0}, {"nv": 0}, {"n": -2}):
        assert group(**kw) == -1 and b"bad sizes" in err()
    assert group(groups=1 << 10, n=1 << 10, nv=1 << 10) == -1 and b"2^31" in err()
    assert group(groups=1 << 20, n=1 << 20, nv=1) == -1 and b"2^31" in err()

    def means(values=p, ptr=(0, 2, 5), idx=p, out=p, rows=2, nv=7, n_regions=None):
        arr = None if ptr is None else (ctypes.c_int32 * len(ptr))(*ptr)
        n_regions = (len(ptr) - 1 if ptr is not None else 2) if n_regions is None else n_regions
        return lib.cfsd_region_means(values, arr, idx, out, rows, nv, n_regions, None)

    for kw in ({"values": None}, {"ptr": None}, {"idx": None}, {"out": None}):
        assert means(**kw) == -1 and b"null" in err()
    for kw in ({"rows": 0}, {"nv": 0}, {"n_regions": 0}, {"rows": -1}):
        assert means(**kw) == -1 and b"bad sizes" in err()
    assert means(ptr=tuple(range(ops.RM_MAX_REGIONS + 2))) == -1 and b"at most" in err()
    assert means(rows=1 << 20, nv=1 << 12) == -1 and b"2^31" in err()
    assert means(ptr=(1, 2, 5)) == -1 and b"expected 0" in err()
    assert means(ptr=(0, 4, 3)) == -1 and b"decreases" in err()
    assert means(ptr=(0, 3, 3)) == -1 and b"empty" in err()
    assert means(ptr=(0, 0, 3)) == -1 and b"empty" in err()


def test_evaluate_constants_match_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cfsd.h")).read()
    assert f"#define CFSD_RM_MAX_REGIONS {ops.RM_MAX_REGIONS}\n" in src
    assert f"#define CFSD_RM_THREADS {ops.RM_THREADS}\n" in src
    assert "#define CFSD_RM_DEPTH(len) (((len) + CFSD_RM_THREADS - 1) / CFSD_RM_THREADS + 9)\n" in src
    assert [ops.region_means_depth(n) for n in (1, 256, 257, 1300, 4096)] == [10, 10, 11, 15, 25]
    assert ops.region_means_depth(4096) <= 32


def test_evaluate_operators_refuse_host_tensors_and_bad_shapes():
    csr = topology.RegionCSR([[0, 1], [4, 2, 1]], 5, device="cpu")
    with pytest.raises(ValueError):
        ops.group_vertex_errors(torch.zeros(4, 5, 3), 2)  # host tensor
    with pytest.raises(ValueError):
        ops.region_means(torch.zeros(2, 5), csr)


# ------------------------------------------------------------------ region CSR
def test_region_csr_layout_and_refusals(topo_npz):
    csr = topology.RegionCSR([[3, 0], [4, 2, 1, 3]], 5, device="cpu")
    assert csr.ptr_host.dtype == np.int32 and csr.ptr_host.tolist() == [0, 2, 6]
    assert csr.ptr.dtype == torch.int32 and csr.ptr.tolist() == [0, 2, 6]
    assert csr.idx.dtype == torch.int32 and csr.idx.tolist() == [3, 0, 4, 2, 1, 3]  # stored order, overlap kept
    assert (csr.n_regions, csr.nnz, csr.nv, csr.lengths) == (2, 6, 5, [2, 4])
    with pytest.raises(ValueError, match="empty"):
        topology.RegionCSR([[0], []], 5, device="cpu")
    with pytest.raises(ValueError, match="outside"):
        topology.RegionCSR([[0, 5]], 5, device="cpu")
    with pytest.raises(ValueError, match="outside"):
        topology.RegionCSR([[-1, 2]], 5, device="cpu")
    with pytest.raises(ValueError):
        topology.RegionCSR([], 5, device="cpu")
    # the template's regions, as DeviceTopology builds them: the lists behind region_mask
    keys = [str(k) for k in topo_npz["region_keys"]]
    regions = [topo_npz[f"region_{i}_feature"] for i in range(len(keys))]
    nv = topo_npz["spiral_0"].shape[0]
    csr = topology.RegionCSR(regions, nv, device="cpu")
    assert csr.n_regions == 15 and csr.nnz == sum(len(r) for r in regions) and max(csr.lengths) <= 4096
    for i, r in enumerate(regions):
        assert csr.idx[csr.ptr_host[i]:csr.ptr_host[i + 1]].tolist() == np.asarray(r).tolist()


def test_topology_region_csr_is_lazy_and_refuses(topo_npz):
    """``DeviceTopology.region_csr``: built on first use from the lists behind
    ``region_mask``; an empty region or an index out of range is refused there
    (a negative index passes the mask's construction by wrapping around)."""
    topo = topology.DeviceTopology.from_npz(topo_npz, device="cpu")
    assert topo._region_csr is None
    csr = topo.region_csr
    assert topo.region_csr is csr and csr.n_regions == topo.n_regions == 15 and csr.nv == topo.n_verts[0]
    mask = np.zeros((csr.n_regions, csr.nv), np.uint8)
    for r in range(csr.n_regions):
        mask[r, csr.idx[csr.ptr_host[r]:csr.ptr_host[r + 1]].numpy()] = 1
    assert np.array_equal(mask, topo.region_mask.numpy())
    for bad in (np.zeros(0, np.int32), np.array([3, -1], np.int32)):
        broken = dict(topo_npz, region_2_feature=bad)
        with pytest.raises(ValueError, match="region 2"):
            topology.DeviceTopology.from_npz(broken, device="cpu").region_csr
    no_regions = {k: v for k, v in topo_npz.items() if not k.startswith("region_")}
    with pytest.raises(ValueError, match="no regions"):
        topology.DeviceTopology.from_npz(no_regions, device="cpu").region_csr
