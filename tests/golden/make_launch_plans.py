"""Generator of ``launch_plans.json``: the libcfsd launch sequence of one eager
train step, per engine configuration (needs an MI355X).

TEST INFRASTRUCTURE.  The fixture pins WHICH entry points a step issues, in
which order and with which integer / float arguments (shapes, workspace byte
counts, the slab geometry of every deferred weight gradient), so a change of
the host code that moves a layer to another kernel, reorders launches or
resizes a workspace region shows as a diff.  Pointers carry no information
beyond null / non-null and are recorded as ``"p"`` / ``"0"``.

    python tests/golden/make_launch_plans.py [--out FILE] [CONFIG ...]

``tests/test_gpu_launch_plan.py`` imports the configurations and the recorder
from here, so the test and the fixture cannot drift apart.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import recipe  # noqa: E402
import synthetic_topology as ST  # noqa: E402

FIXTURE = os.path.join(HERE, "launch_plans.json")

# the body configuration of test_c4_body
W_BODY = {"kl": 0.0, "lc": 1.0, "lap": 1.0}
BODY_CH, BODY_LATENT = [32, 32, 64], 33
# the small non-selection torus: levels 288 / 144 / 72 / 36
SMALL = dict(nu=24, nv=12, factors=(2, 2, 2))
AVERAGED = {"all": (0, 1, 2), "mixed": (1,)}   # levels whose Pool(down) is no selection

# name -> (topology, engine keywords, fuse_bottleneck, no-op grad hook, batch)
CONFIGS = {
    "a": ("cranio", {}, True, False, 16),
    "b": ("cranio", {"vertex_major": False}, True, False, 16),
    "c": ("cranio", {"precision": "bf16"}, True, False, 16),
    "d": ("cranio", {}, True, True, 16),
    "e": ("cranio", {}, False, False, 16),
    "f": ("cranio", {"swap_features": False}, True, False, 4),
    "g": ("torus", {}, True, False, 16),
    "h": ("small-all", {}, False, False, 16),
    "i": ("small-mixed", {}, False, False, 16),
}

_npz = {}


def topology_npz(name):
    """The hierarchy arrays of a configuration's topology (cached)."""
    if name not in _npz:
        if name == "cranio":
            _npz[name] = recipe.load_topology()
        elif name == "torus":
            _npz[name] = ST.torus_topology()
        else:
            if "small" not in _npz:
                _npz["small"] = ST.torus_topology(**SMALL)
            _npz[name] = ST.averaging_down(_npz["small"], AVERAGED[name.split("-")[1]])
    return _npz[name]


def body_weights(num_vert):
    shapes = recipe.param_shapes(num_vert=num_vert, out_ch=BODY_CH, latent=BODY_LATENT, is_vae=False)
    return recipe.golden_weights(shapes, seed=4)


def meshes_of(topo_name, n, seed=0):
    if topo_name == "cranio":
        m = recipe.normalized_meshes()
        return m[np.arange(n) % len(m)]
    if topo_name == "torus":
        return ST.torus_meshes(n, seed=seed)
    return ST.torus_meshes(n, nu=SMALL["nu"], nv=SMALL["nv"], seed=seed)


class NoopHook:
    """A bucketed gradient hook that does nothing (the ``split=True`` backward)."""

    def bucket_ready(self, grad):
        pass

    def finish(self, grad):
        pass


def make_engine(name, device="cuda"):
    """(engine, device topology) of configuration ``name``, golden weights loaded."""
    import cfsd_loader
    cfsd_loader.load()
    from craniofacialsd_vae_amd import engine as E
    from craniofacialsd_vae_amd import topology
    topo_name, kw, fuse_bn, _, _ = CONFIGS[name]
    dtopo = topology.DeviceTopology.from_npz(topology_npz(topo_name), device=device)
    if topo_name == "cranio":
        eng = E.SDVAEEngine(dtopo, E.ModelSpec(), swap_bs=4, device=device, **kw)
        w = recipe.golden_weights()
    else:
        eng = E.SDVAEEngine(dtopo, E.ModelSpec(3, BODY_CH, BODY_LATENT, is_vae=False), w_kl=W_BODY["kl"],
                            w_lc=W_BODY["lc"], w_lap=W_BODY["lap"], swap_bs=4, device=device, **kw)
        w = body_weights(dtopo.n_verts[-1])
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    if not fuse_bn:
        eng.fuse_bottleneck = False
    return eng, dtopo


def _token(a):
    if a is None:
        return "0"
    if isinstance(a, ctypes.c_void_p):
        return "p" if a.value else "0"
    if isinstance(a, ctypes.Array):  # cfsd_dw_slabs[]: the int fields of every item
        return [[s.batch, s.vsrc, s.rows, s.cin, s.cout, s.fused] for s in a]
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    raise TypeError(f"launch argument of type {type(a).__name__}")


def canonical(records):
    """``_abi.trace_launches`` records as ``[[name, tokens], ...]``."""
    return [[name, [_token(a) for a in args]] for name, args, _, _ in records]


def record_step(name, eng):
    """One warm-up step, then the canonical record of one eager step."""
    from craniofacialsd_vae_amd import _abi
    topo_name, _, _, hook, bsz = CONFIGS[name]
    b = eng.set_batch(torch.from_numpy(meshes_of(topo_name, bsz)).to(eng.device), key_index=2)
    hook = NoopHook() if hook else None
    eng.train_step_on(b, grad_hook=hook)
    torch.cuda.synchronize()
    with _abi.trace_launches() as rec:
        eng.train_step_on(b, grad_hook=hook)
    torch.cuda.synchronize()
    return canonical(rec)


def dumps(plans):
    """One launch per line (a readable diff when a plan changes)."""
    out = ["{"]
    names = sorted(plans)
    for i, name in enumerate(names):
        out.append(f' "{name}": [')
        rows = plans[name]
        out += ["  " + json.dumps(r) + ("," if k + 1 < len(rows) else "") for k, r in enumerate(rows)]
        out.append(" ]" + ("," if i + 1 < len(names) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


def load_fixture(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("configs", nargs="*", help="configurations to record (default: all)")
    args = ap.parse_args(argv)
    plans = {}
    for name in args.configs or sorted(CONFIGS):
        eng, _ = make_engine(name)
        plans[name] = record_step(name, eng)
        print(f"{name}: {len(plans[name])} launches")
    with open(args.out, "w") as f:
        f.write(dumps(plans))


if __name__ == "__main__":
    main()
