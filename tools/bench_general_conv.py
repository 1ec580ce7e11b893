"""``python tools/bench_general_conv.py [--out FILE]``: the general-shape
SpiralConv kernels (``cfsd_spiral_conv_gen_*``) against the reference's own
algorithm, one JSON line, printed and written to
``profiles/general_conv_bench.json`` (or ``FILE``; ``--out ''`` only prints).

Forward, data gradient (dx) and weight gradient (dW, db) of one full conv at
the craniofacial level sizes (17 039 / 4 260 / 1 065 vertices, batch 16,
fp32), in ONE process on one GPU:

* ``gen``: ``ops.spiral_conv_fwd`` / ``_bwd_data`` / ``_bwd_weight`` (the
  immediate form, slab reduce included) on the general kernels;
* ``torch``: the reference's composed ``index_select`` + ``addmm``
  (``model.py:27-41``) and its autograd (``torch.autograd.grad`` of the
  retained forward graph w.r.t. x alone for dx, w.r.t. weight and bias for dW);
* ``spec`` (context shapes only): the specialised kernels of the same entry
  points, next to ``gen`` forced onto their shapes.

The spiral tables come from the craniofacial template (length 9): a length-7
table keeps the first 7 columns, a length-12 one appends columns 1..3 of the
spiral of each row's last vertex, so the gathers keep a mesh's locality.

A timing is device events around ``--iters`` back-to-back calls; the
implementations of one (shape, level, product) alternate, the order flipping
every repeat, after ``--warmup`` untimed rounds; ``*_us`` is the median over
``--repeats`` (>= 5) repeats, ``*_us_min`` / ``*_us_max`` the spread.
``slower_than_torch`` lists the (shape, level, product) triples where ``gen``
is slower than ``torch``: the pass criterion is that it is empty.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

SHAPES = [(12, 32, 32), (9, 48, 48), (7, 24, 40)]  # (seq, cin, cout) without a specialised instance
CONTEXT = [(9, 32, 32), (9, 64, 64)]               # specialised shapes, general family forced on
BATCH = 16


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed repeat")
    ap.add_argument("--levels", type=int, default=3, help="template levels measured (finest first)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_conv_bench.json"),
                    help="file that receives the line ('' = none)")
    opts = ap.parse_args(argv)
    if opts.repeats < 5:
        ap.error("--repeats must be at least 5")

    import numpy as np
    import torch

    import cfsd_loader
    import recipe
    cfsd_loader.load()
    from craniofacialsd_vae_amd import ops, topology

    if not torch.cuda.is_available():
        raise RuntimeError("bench_general_conv measures on the GPU; no GPU visible")
    dev = torch.device("cuda", 0)
    npz = recipe.load_topology()
    g = torch.Generator().manual_seed(0)

    def table(level, seq):
        sp = np.asarray(npz[f"spiral_{level}"], np.int64)
        if seq <= sp.shape[1]:
            return np.ascontiguousarray(sp[:, :seq])
        assert seq - sp.shape[1] < sp.shape[1]
        return np.concatenate([sp, sp[sp[:, -1]][:, 1:1 + seq - sp.shape[1]]], 1)

    def case(level, seq, cin, cout):
        idx = table(level, seq)
        nv = idx.shape[0]
        c = {"idx": torch.from_numpy(idx.astype(np.int32)).to(dev), "idx64": torch.from_numpy(idx.reshape(-1)).to(dev),
             "inv": tuple(torch.from_numpy(a).to(dev) for a in topology.inverse_spiral(idx, nv)), "nv": nv,
             "x": torch.randn(BATCH, nv, cin, generator=g).to(dev),
             "w": (torch.randn(cout, seq * cin, generator=g) / (seq * cin) ** 0.5).to(dev),
             "b": torch.randn(cout, generator=g).to(dev), "dy": torch.randn(BATCH, nv, cout, generator=g).to(dev)}
        return c

    def library(c, seq, cin, cout, general):
        kw = {"general": True} if general else {}
        y, dx = torch.empty_like(c["dy"]), torch.empty_like(c["x"])
        dw, db = torch.empty_like(c["w"]), torch.empty_like(c["b"])
        ws = torch.empty(max(ops.spiral_conv_bwd_weight_workspace(BATCH, c["nv"], seq, cin, cout, **kw),
                             ops.spiral_conv_workspace(BATCH, c["nv"], c["nv"], seq, cin, cout)) // 4 + 64,
                         dtype=torch.float32, device=dev)
        return {"fwd": lambda: ops.spiral_conv_fwd(c["x"], c["idx"], c["w"], c["b"], ops.ACT_NONE, out=y, workspace=ws,
                                                   **kw),
                "dx": lambda: ops.spiral_conv_bwd_data(c["dy"], c["inv"], c["w"], c["nv"], out=dx, workspace=ws, **kw),
                "dw": lambda: ops.spiral_conv_bwd_weight(c["x"], c["idx"], c["dy"], dw, db, ws, **kw)}, (y, dx, dw, db)

    def reference(c):
        x, w, b = (c[k].clone().requires_grad_(True) for k in ("x", "w", "b"))

        def fwd():
            G = torch.index_select(x, 1, c["idx64"]).view(BATCH * c["nv"], -1)
            return torch.addmm(b, G, w.t()).view(BATCH, c["nv"], -1)

        y = fwd()
        return {"fwd": lambda: fwd().detach(),
                "dx": lambda: torch.autograd.grad(y, x, c["dy"], retain_graph=True)[0],
                "dw": lambda: torch.autograd.grad(y, (w, b), c["dy"], retain_graph=True)}, y

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(opts.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / opts.iters * 1e3  # us per call

    def compare(impls):
        """{name: fn} -> {name: (median, min, max)} us, alternating, order flipping every repeat."""
        names = list(impls)
        for _ in range(opts.warmup):
            for n in names:
                timed(impls[n])
        t = {n: [] for n in names}
        for r in range(opts.repeats):
            for n in (names if r % 2 == 0 else names[::-1]):
                t[n].append(timed(impls[n]))
        return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}

    rows, slower = [], []
    for context, shapes in ((False, SHAPES), (True, CONTEXT)):
        for (seq, cin, cout) in shapes:
            for level in range(opts.levels):
                c = case(level, seq, cin, cout)
                gen, out_gen = library(c, seq, cin, cout, general=True)
                ref, y_ref = reference(c)
                spec = library(c, seq, cin, cout, general=False)[0] if context else None
                # same results first (fp32 sums in another order: 1e-4 of the output's scale)
                gen["fwd"](), gen["dx"](), gen["dw"]()
                dx_ref, (dw_ref, db_ref) = ref["dx"](), ref["dw"]()
                for got, want in zip(out_gen, (y_ref.detach(), dx_ref, dw_ref, db_ref)):
                    err = float((got - want).abs().max() / (1.0 + want.abs().max()))
                    if not err < 1e-4:
                        raise RuntimeError(f"general kernels differ from torch at {(seq, cin, cout)} level {level}: {err}")
                for prod in ("fwd", "dx", "dw"):
                    impls = {"gen": gen[prod], "torch": ref[prod]}
                    if spec is not None:
                        impls["spec"] = spec[prod]
                    res = compare(impls)
                    row = {"shape": [seq, cin, cout], "rows": c["nv"], "product": prod, "context": context}
                    for n, (med, lo, hi) in res.items():
                        row[f"{n}_us"], row[f"{n}_us_min"], row[f"{n}_us_max"] = round(med, 1), round(lo, 1), round(hi, 1)
                    rows.append(row)
                    if not context and res["gen"][0] > res["torch"][0]:
                        slower.append([[seq, cin, cout], c["nv"], prod])
                del c, gen, ref, spec, out_gen, y_ref
    res = {"bench": "general_conv", "device": torch.cuda.get_device_name(0), "batch": BATCH, "repeats": opts.repeats,
           "iters_per_repeat": opts.iters, "results": rows, "slower_than_torch": slower}
    line = json.dumps(res)
    print(line)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
