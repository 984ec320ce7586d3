"""Writes tests/golden/curves_ref.npz: sklearn's float64 answers for the curves module, on two inputs.

    fixture  logits / target of tests/golden/seg_metrics_ref.npz (2 x 23 x 24 x 40; targets outside [0, 23) are left out)
    sharp    tests/_curves_ref.sharp_case(): 2 x 23 x 64 x 64, seeded, stored in the file as int16 multiples of 1/256

Per input and class, from sklearn.metrics in float64: roc_auc_score and average_precision_score of the EXACT score and of the
BIN INDEX (the quantised score), and roc_curve / precision_recall_curve of the bin index (variable length: concatenated, with
offsets).  Classes without positives (or negatives) carry NaN and empty curves.  Needs scikit-learn; no test imports it.

    python tools/gen_curves_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _curves_ref as R  # noqa: E402


def answers(logits, target):
    from sklearn import metrics as sk
    s = R.scores(logits)
    c = s.shape[1]
    t = np.asarray(target).reshape(-1)
    valid = (t >= 0) & (t < c)
    s, t = s[valid], t[valid]
    b = R.bin_index(s)
    out = {k: np.full(c, np.nan) for k in ("auc_exact", "ap_exact", "auc_bin", "ap_bin")}
    roc, pr = [], []
    for k in range(c):
        y = t == k
        if y.any():
            # +inf scores (a probability that rounds to 1 in float64) are legal for a rank statistic but not for sklearn's input check
            sk_s = np.clip(s[:, k], -1e300, 1e300)
            out["ap_exact"][k] = sk.average_precision_score(y, sk_s)
            out["ap_bin"][k] = sk.average_precision_score(y, b[:, k])
        if y.any() and not y.all():
            out["auc_exact"][k] = sk.roc_auc_score(y, sk_s)
            out["auc_bin"][k] = sk.roc_auc_score(y, b[:, k])
            fpr, tpr, thr = sk.roc_curve(y, b[:, k])
            roc.append(np.stack([fpr, tpr, thr]))
            p, r, th = sk.precision_recall_curve(y, b[:, k])
            pr.append(np.stack([p[:-1], r[:-1], th.astype(np.float64)]))      # the closing (1, 0) point has no threshold
        else:
            roc.append(np.zeros((3, 0)))
            pr.append(np.zeros((3, 0)))
    out["roc"] = np.concatenate(roc, axis=1)
    out["roc_offsets"] = np.cumsum([0] + [a.shape[1] for a in roc]).astype(np.int64)
    out["pr"] = np.concatenate(pr, axis=1)
    out["pr_offsets"] = np.cumsum([0] + [a.shape[1] for a in pr]).astype(np.int64)
    return out


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "seg_metrics_ref.npz"))
    q, st = R.sharp_case()
    data = {"sharp_logits_q": q, "sharp_target": st.astype(np.uint8), "bins": np.int64(R.SCORE_BINS),
            "score_range": np.float64(R.SCORE_RANGE)}
    for name, (lg, tg) in {"fixture": (g["logits"], g["target"]), "sharp": (q.astype(np.float32) / 256.0, st)}.items():
        for k, v in answers(lg, tg).items():
            data[f"{name}/{k}"] = v
        s = R.scores(lg)
        print(name, "classes present:", int(np.isfinite(data[f"{name}/ap_exact"]).sum()), "score range:", float(s[np.isfinite(s)].min()),
              float(s[np.isfinite(s)].max()), "max |auc_bin - auc_exact|:", float(np.nanmax(np.abs(data[f"{name}/auc_bin"] - data[f"{name}/auc_exact"]))))
    path = os.path.join(ROOT, "tests", "golden", "curves_ref.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
