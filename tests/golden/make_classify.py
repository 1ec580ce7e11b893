"""Records what scikit-learn computes on the seeded classifier cases
(``classify_cases.py``) into ``classify_sklearn.npz``: run by hand on a machine
with scikit-learn (``python tests/golden/make_classify.py``); the tests read
the file and never import scikit-learn.

Per case, from ``LinearDiscriminantAnalysis(n_components=2,
store_covariance=True)`` and ``QuadraticDiscriminantAnalysis(
store_covariance=True)`` fitted in float64 on the training rows with a label in
range and evaluated on the held-out rows: decision values, predictions, means
and priors of both, LDA's log-probabilities and 2-D transform.

Also asserts what the tests rely on: at most 2 % of the held-out rows have a
top-two margin within twice the tests' score tolerance (1e-4 of the largest
reference score), and every class covariance is well-conditioned.
"""
import os

import numpy as np
from sklearn.discriminant_analysis import LinearDiscriminantAnalysis, QuadraticDiscriminantAnalysis

import classify_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


def margins(dec):
    top = np.sort(dec, axis=1)
    return top[:, -1] - top[:, -2]


def main():
    out = {}
    for name in cases.CASES:
        case = cases.make_case(name)
        x, y = cases.valid_rows(case)
        col0, d = case["cols"]
        xt = case["zt"][:, col0:col0 + d].astype(np.float64)
        lda = LinearDiscriminantAnalysis(n_components=2, store_covariance=True).fit(x, y)
        qda = QuadraticDiscriminantAnalysis(store_covariance=True).fit(x, y)
        rec = {"lda_decision": lda.decision_function(xt), "lda_log_proba": lda.predict_log_proba(xt),
               "lda_pred": lda.predict(xt).astype(np.int32), "lda_transform": lda.transform(xt),
               "lda_means": lda.means_, "lda_priors": lda.priors_,
               "qda_decision": qda.decision_function(xt), "qda_pred": qda.predict(xt).astype(np.int32),
               "qda_means": qda.means_, "qda_priors": qda.priors_}
        for kind in ("lda", "qda"):
            dec = rec[f"{kind}_decision"]
            ref = dec - dec.mean(1, keepdims=True) if kind == "lda" else dec
            tol = 1e-4 * np.abs(ref).max()
            close = float((margins(dec) <= 2 * tol).mean())
            assert close <= 0.02, (name, kind, close)
            print(f"{name} {kind}: max|score| {np.abs(ref).max():.4g}, smallest margin {margins(dec).min():.3g}, "
                  f"{100 * close:.2f} % of rows within the margin rule, "
                  f"accuracy {(rec[f'{kind}_pred'] == case['yt']).mean():.3f}")
        conds = [np.linalg.cond(c) for c in qda.covariance_]
        assert max(conds) < 1e4, (name, conds)
        print(f"{name}: class covariance condition numbers {[round(c) for c in conds]}")
        out.update({f"{name}.{k}": v for k, v in rec.items()})
    path = os.path.join(HERE, "classify_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
