"""Float64 NumPy restatement of the pixel AUROC / AUPRC that ops.BinaryAUC computes on the device (the semantics of
roc_auc_score and auc(precision_recall_curve) in the reference src/utils.py:84-91).

Over the pixels with P positives (truth > 0.5) and N negatives, grouping equal scores (float equality, -0.0 == +0.0):
    AUROC = sum_v pos_v (2 #neg<v + neg_v) / (2 P N)             (exact integer numerator, one rounding)
    AUPRC = sum_{v: pos_v > 0} pos_v / P (prec(>= v) + prec(> v)) / 2,   prec(> v) = 1 when nothing lies above v
No positives, no negatives or any NaN / inf score: 0.0 / 0.0 (calculate_metrics when sklearn refuses).
Plain helper module: test_cpu_rank_auc.py pins it against sklearn, test_gpu_rank_auc.py holds the kernels to it.
"""
import numpy as np


def rank_auc64(scores, positive):
    s = np.asarray(scores, dtype=np.float32).ravel()
    y = np.asarray(positive, dtype=bool).ravel()
    finite = np.isfinite(s)
    nonfinite = int((~finite).sum())
    pos = np.sort(s[finite & y].astype(np.float64) + 0.0)          # + 0.0: -0.0 becomes +0.0
    neg = np.sort(s[finite & ~y].astype(np.float64) + 0.0)
    P, N = int(pos.size), int(neg.size)
    res = {"auroc": 0.0, "auprc": 0.0, "positives": P, "negatives": N, "nonfinite": nonfinite}
    if nonfinite or P == 0 or N == 0:
        return res
    v, first, cnt = np.unique(pos, return_index=True, return_counts=True)
    lo = np.searchsorted(neg, v, "left")
    hi = np.searchsorted(neg, v, "right")
    nv = hi - lo
    num = int(np.sum(cnt.astype(np.int64) * (2 * lo.astype(np.int64) + nv)))
    res["auroc"] = num / (2 * P * N)                                # Python int / int: correctly rounded
    above_p = P - (first + cnt)
    above_n = N - hi
    cur = (above_p + cnt) / (above_p + cnt + above_n + nv)
    prev = np.where(above_p + above_n > 0, above_p / np.maximum(above_p + above_n, 1), 1.0)
    res["auprc"] = float(np.sum(cnt / P * ((cur + prev) / 2)))
    return res
