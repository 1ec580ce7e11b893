"""Records what the reference's planning arithmetic gives on the seeded
classifier cases (``classify_cases.py``) into ``planning_scipy.npz``: run by
hand on a machine with scipy and scikit-learn (``python
tests/golden/make_planning.py``; made with scipy 1.15.3, scikit-learn 1.7.2);
the tests read the file and never import either.

Per case (``full75``, ``region5``, ``odd20``): the healthy class is class 0 of
a float64 ``QuadraticDiscriminantAnalysis(store_covariance=True)`` on the
training rows, the patients are the held-out rows.  As ``test.py:663-704``
does, ``scipy.stats.multivariate_normal.logpdf`` is evaluated on every point of
the 5000-point ``torch.linspace`` grid from the patient to the healthy mean and
compared with the logpdf of the aligned distribution at 3, 2 and 1 standard
deviations.  Stored: ``mean``, ``whiten`` (``V / sqrt(w)`` of ``eigh`` of the
covariance, what ``classify.finish_qda`` makes), the first index per level,
each crossing's ``margin = min(level - maha(i), maha(i - 1) - level) / level``
(float64 Mahalanobis distances of the grid points; only the first term for
``i = 0``) and the patient's own distance.

For ``full75`` also the pre- / post-operative quantities of
``test.py:992-1081`` for 128 pairs (held-out rows ``i`` and ``128 + i``) over
16 windows, the whole latent and its 15 five-column regions, each with its own
QDA: the six raw quantities from ``scipy.spatial.distance.mahalanobis`` /
``euclidean`` with ``np.linalg.inv`` of the float64 covariance, the composed
metrics, and the packed ``mean`` / ``whiten`` of the windows.

Asserts what the tests rely on: at most 5 % of a case's crossings lie within
the margin rule (1e-5), ``region5`` has patients inside 3 sigma, and the closed
form of ``csrc/planning.hip`` (restated in numpy on fp32-stored parameters)
gives the recorded index on every crossing outside the margin rule.
"""
import os

import numpy as np
import torch
from scipy.linalg import eigh
from scipy.spatial.distance import euclidean, mahalanobis
from scipy.stats import multivariate_normal
from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis

import classify_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 5000
LEVELS = (3.0, 2.0, 1.0)
MARGIN = 1e-5
N_PAIRS = 128
PROCEDURE = (1, 4, 8)  # windows of the recorded procedure_metric (regions 0, 3 and 7)


def healthy(x, y):
    qda = QuadraticDiscriminantAnalysis(store_covariance=True).fit(x, y)
    mean, cov = qda.means_[0], qda.covariance_[0]
    w, v = np.linalg.eigh(cov)
    return mean, cov, v / np.sqrt(w)


def grid_of(z_row, mean):
    """``Tester.vector_linspace(z_p, z_mean_target, 5000)``: fp32 columns."""
    cols = [torch.linspace(float(s), float(f), STEPS) for s, f in zip(z_row, mean)]
    return torch.stack(cols).t().numpy()


def closed_form(z, mean, whiten):
    """numpy restatement of cfsd_plan_targets on fp32-stored parameters."""
    mean32, wh = mean.astype(np.float32), whiten.astype(np.float32).astype(np.float64)
    s, e = z.astype(np.float32), mean32[None]
    step = (e - s) / np.float32(STEPS - 1)

    def maha_at(i):  # i [n] -> distance of grid point i of every row
        i = i[:, None]
        g = np.where(i < STEPS // 2, s + step * i.astype(np.float32), e - step * (STEPS - 1 - i).astype(np.float32))
        assert g.dtype == np.float32
        return np.sqrt((((g.astype(np.float64) - mean32.astype(np.float64)) @ wh) ** 2).sum(1))

    m0 = maha_at(np.zeros(len(z), np.int64))
    out = np.empty((len(z), len(LEVELS)), np.int64)
    for k, level in enumerate(LEVELS):
        with np.errstate(divide="ignore"):
            i0 = np.clip(np.ceil((STEPS - 1) * (1.0 - level / m0)), 0, STEPS - 1).astype(np.int64)
        found = np.minimum(i0 + 1, STEPS - 1)
        for t in (1, 0, -1):
            i = i0 + t
            ok = (i >= 0) & (i <= STEPS - 1)
            inside = maha_at(np.clip(i, 0, STEPS - 1)) <= level
            found = np.where(ok & inside, i, found)
        out[:, k] = found
    return out


def crossings(name):
    case = cases.make_case(name)
    x, y = cases.valid_rows(case)
    col0, d = case["cols"]
    mean, cov, whiten = healthy(x, y)
    z = case["zt"][:, col0:col0 + d]
    dist = multivariate_normal(mean=mean, cov=cov)
    eigenval, _ = eigh(cov)
    reference = multivariate_normal(mean=np.zeros_like(mean), cov=np.diag(eigenval))
    std_vec = np.zeros_like(mean)
    std_vec[0] = np.sqrt(reference.cov[0, 0])
    thresholds = [-reference.logpdf(level * std_vec) for level in LEVELS]
    n = len(z)
    index, margin = np.empty((n, 3), np.int32), np.empty((n, 3))
    for p in range(n):
        grid = grid_of(z[p], mean)
        pdf = -dist.logpdf(grid)
        maha = np.sqrt((((grid.astype(np.float64) - mean) @ whiten) ** 2).sum(1))
        for k, (level, thr) in enumerate(zip(LEVELS, thresholds)):
            i = int(np.argmax(pdf <= thr))
            assert pdf[i] <= thr
            index[p, k] = i
            margin[p, k] = min(level - maha[i], maha[i - 1] - level if i else np.inf) / level
    maha0 = np.sqrt((((z.astype(np.float64) - mean) @ whiten) ** 2).sum(1))
    excluded = float((margin <= MARGIN).mean())
    assert excluded <= 0.05, (name, excluded)
    mine = closed_form(z, mean, whiten)
    clear = margin > MARGIN
    assert np.array_equal(mine[clear], index[clear]) and np.abs(mine - index).max() <= 1, name
    print(f"{name}: {n} patients, {100 * excluded:.1f} % of the crossings within the margin rule, "
          f"{int((index[:, 0] == 0).sum())} patients inside 3 sigma, closed form equal on "
          f"{int(clear.sum())} crossings, distance {maha0.min():.2f}..{maha0.max():.2f}")
    return {"mean": mean, "whiten": whiten, "index": index, "margin": margin, "maha": maha0}


def pairs():
    case = cases.make_case("full75")
    x, y = cases.valid_rows(case)
    zt = case["zt"].astype(np.float64)
    windows = [(0, 75)] + [(5 * r, 5) for r in range(15)]
    table, means, whitens, raw = [], [], [], np.empty((N_PAIRS, len(windows), 6))
    for w, (col0, d) in enumerate(windows):
        mean, cov, whiten = healthy(x[:, col0:col0 + d], y)
        table.append((col0, d, sum(len(m) for m in means), sum(len(m) for m in whitens)))
        means.append(mean)
        whitens.append(whiten.reshape(-1))
        inv = np.linalg.inv(cov)
        for p in range(N_PAIRS):
            pre, post = zt[p, col0:col0 + d], zt[N_PAIRS + p, col0:col0 + d]
            displacement, ideal = post - pre, mean - pre
            cos = np.dot(displacement / np.linalg.norm(displacement), ideal / np.linalg.norm(ideal))
            raw[p, w] = (mahalanobis(pre, mean, inv), mahalanobis(post, mean, inv), euclidean(pre, mean),
                         euclidean(post, mean), cos, mahalanobis(post, pre, inv))
    distances = (raw[..., 0] - raw[..., 1]) / raw[..., 1]
    with_angle = raw[..., 5] * raw[..., 4] / raw[..., 1]
    l2 = (raw[:, 0, 2] - raw[:, 0, 3]) / raw[:, 0, 3]
    procedure = distances[:, list(PROCEDURE)].sum(1) / len(PROCEDURE)
    print(f"pairs: raw {raw.min():.3g}..{raw.max():.3g}, global metric {distances[:, 0].min():.3g}.."
          f"{distances[:, 0].max():.3g}")
    return {"windows": np.array(table, np.int32), "mean": np.concatenate(means), "whiten": np.concatenate(whitens),
            "raw": raw, "metric_distances": distances, "metric_with_angle": with_angle, "global_metric_l2": l2,
            "procedure_metric": procedure, "procedure_windows": np.array(PROCEDURE, np.int32)}


def main():
    out = {}
    for name in ("full75", "region5", "odd20"):
        out.update({f"{name}.{k}": v for k, v in crossings(name).items()})
    assert (out["region5.index"][:, 0] == 0).any()
    out.update({f"pairs.{k}": v for k, v in pairs().items()})
    path = os.path.join(HERE, "planning_scipy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
