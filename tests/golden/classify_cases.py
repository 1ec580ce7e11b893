"""Seeded inputs of the classifier tests (``test_gpu_classify.py``,
``test_classify_host.py``) and of ``make_classify.py``, which records what
scikit-learn computes on them.  Inputs are regenerated from the seed, never
stored.

Each case: training latents ``z`` [n, ld] float32 with labels ``y`` (int32),
the column window ``cols = (col0, d)`` the classifiers read, and held-out rows
``zt`` [64 C, ld] with labels ``yt``.  Classes are Gaussians with their own
mean and covariance (condition number ``cond``: well-conditioned, as QDA on
fewer than a few d rows per class is ill-posed in any implementation).
"""
import numpy as np

CASES = {
    # name: (class sizes, ld, col0, d, planted out-of-range labels, separation, cond, seed)
    "full75": ((700, 600, 500, 450), 75, 0, 75, 0, 0.6, 100.0, 11),
    "region5": ((50, 45, 45, 40), 75, 70, 5, 0, 0.8, 40.0, 12),     # the last region's window
    "odd20": ((34, 31, 29), 20, 0, 20, 1, 0.8, 10.0, 13),           # n = 95 with one out-of-range label
}
HELD_OUT = 64  # rows per class


def make_case(name):
    sizes, ld, col0, d, n_bad, sep, cond, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n_cls = len(sizes)
    means = rng.normal(0.0, sep, (n_cls, d))
    mix = []
    for _ in range(n_cls):
        q = np.linalg.qr(rng.normal(size=(d, d)))[0]
        s = 0.3 * np.sqrt(np.logspace(0.0, np.log10(cond), d))
        mix.append((q * s) @ q.T)

    def draw(counts):
        y = np.concatenate([np.full(m, c) for c, m in enumerate(counts)])
        x = np.concatenate([means[c] + rng.normal(size=(m, d)) @ mix[c] for c, m in enumerate(counts)])
        full = rng.normal(0.0, 1.0, (len(y), ld))
        full[:, col0:col0 + d] = x
        order = rng.permutation(len(y))
        return full[order].astype(np.float32), y[order].astype(np.int32)

    z, y = draw(sizes)
    zt, yt = draw((HELD_OUT,) * n_cls)
    if n_bad:  # extra rows whose label is out of range: they must contribute to nothing
        zb = rng.normal(0.0, 3.0, (n_bad, ld)).astype(np.float32)
        at = int(rng.integers(1, len(y) - 1))
        z = np.concatenate([z[:at], zb, z[at:]])
        y = np.concatenate([y[:at], np.full(n_bad, n_cls, np.int32), y[at:]])
    return {"z": z, "y": y, "zt": zt, "yt": yt, "cols": (col0, d), "n_classes": n_cls}


def valid_rows(case):
    """Training rows with a label in range, as float64 window columns."""
    col0, d = case["cols"]
    keep = (case["y"] >= 0) & (case["y"] < case["n_classes"])
    return case["z"][keep, col0:col0 + d].astype(np.float64), case["y"][keep]
