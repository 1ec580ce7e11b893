"""Records scikit-learn's answers for ``evaluation.classification_report`` /
``evaluation.confusion_matrix`` into ``evaluate_sklearn.json`` (run on the CPU
with scikit-learn 1.7.2; the tests read only the JSON).

Cases: an ordinary four-class vector; a class that is predicted but absent
from the truth; a true class that is never predicted; one single class;
integer labels; everything wrong."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    rs = np.random.RandomState(11)
    four = rs.choice(list("acmn"), size=60).tolist()
    noisy = [t if rs.rand() < 0.7 else "acmn"[rs.randint(4)] for t in four]
    return {
        "four_classes": (four, noisy),
        "predicted_but_absent": (list("ccmmnnnmc"), list("camanncmc")),   # 'a' only among the predictions
        "never_predicted": (list("aacmnnmca"), list("ccccnnmcm")),        # 'a' only in the truth
        "single_class": (list("nnnnn"), list("nnnnn")),
        "integers": ([0, 2, 2, 1, 0, 3, 3, 1, 2, 0], [0, 2, 1, 1, 0, 3, 0, 1, 2, 2]),
        "all_wrong": (list("aacc"), list("ccaa")),
    }


def main():
    import warnings

    import sklearn
    from sklearn.metrics import classification_report, confusion_matrix
    from sklearn.utils.multiclass import unique_labels
    out = {"sklearn": sklearn.__version__, "cases": {}}
    for name, (y_true, y_pred) in cases().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # UndefinedMetricWarning: the zero denominators are the point
            report = classification_report(y_true, y_pred, output_dict=True)
            cm = confusion_matrix(y_true, y_pred, normalize="true")
        out["cases"][name] = {
            "y_true": y_true, "y_pred": y_pred,
            "report": json.loads(json.dumps(report, default=lambda v: v.item())),
            "labels": [v.item() if isinstance(v, np.generic) else v for v in unique_labels(y_true, y_pred)],
            "confusion_true": cm.tolist(),
            "confusion_counts": confusion_matrix(y_true, y_pred).tolist(),
        }
    with open(os.path.join(HERE, "evaluate_sklearn.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {len(out['cases'])} cases, scikit-learn {sklearn.__version__}")


if __name__ == "__main__":
    main()
