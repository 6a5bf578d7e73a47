"""Float64 restatements for the ranking scores (no torch, no project code):

  * rank_counts: the four integers per row (n_ge, p_ge, n_gt, p_gt) by plain loops, as include/m2mixer.h defines them;
  * average_precision / roc_auc: the two scores of one class FROM A SORT, the way torchmetrics and scikit-learn compute them
    (distinct thresholds in descending order, cumulative true / false positives) -- independent of the count formulas of
    m2_mixer_amd/scores.py;
  * rank_from_scores: per-class and macro values of a (n, K) score matrix, with the macro rule of scores.rank_scores;
  * softmax64: the softmax of float32 logits in float64.
"""
import numpy as np


def rank_counts(probs, labels, K):
    """probs (K, n) class columns of ONE head, labels (n) with -1 = no label -> (n, 4) int64."""
    probs, labels = np.asarray(probs), np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        y = int(labels[i])
        if y < 0 or y >= K:
            continue
        s = probs[y][i]
        for j in range(n):
            lj = int(labels[j])
            if lj < 0 or lj >= K:
                continue
            v = probs[y][j]
            same = lj == y
            if v >= s:
                out[i, 0] += 1
                out[i, 1] += same
            if v > s:
                out[i, 2] += 1
                out[i, 3] += same
    return out


def rank_counts_fast(probs, labels, K):
    """The same integers with numpy comparisons per row (for the larger GPU cases; checked against rank_counts in the CPU tests)."""
    probs, labels = np.asarray(probs), np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((n, 4), dtype=np.int64)
    ok = (labels >= 0) & (labels < K)
    for i in range(n):
        y = int(labels[i])
        if not ok[i]:
            continue
        col = probs[y]
        with np.errstate(invalid="ignore"):
            ge, gt = ok & (col >= col[i]), ok & (col > col[i])
        same = labels == y
        out[i] = (ge.sum(), (ge & same).sum(), gt.sum(), (gt & same).sum())
    return out


def _curve(scores, positive):
    """Distinct thresholds in descending order -> cumulative (tp, fp) after each one (ties share a threshold)."""
    scores, positive = np.asarray(scores, dtype=np.float64), np.asarray(positive, dtype=bool)
    order = np.argsort(-scores, kind="stable")
    s, p = scores[order], positive[order]
    last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]          # last index of every tie group
    tp = np.cumsum(p)[last].astype(np.float64)
    fp = np.cumsum(~p)[last].astype(np.float64)
    return tp, fp


def average_precision(scores, positive):
    """sum over thresholds of (recall_k - recall_{k-1}) * precision_k; NaN without positives."""
    positive = np.asarray(positive, dtype=bool)
    P = int(positive.sum())
    if P == 0 or len(positive) == 0:
        return float("nan")
    tp, fp = _curve(scores, positive)
    recall, precision = tp / P, tp / (tp + fp)
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def roc_auc(scores, positive):
    """Trapezoidal area under (fpr, tpr) over the distinct thresholds; NaN without positives or without negatives."""
    positive = np.asarray(positive, dtype=bool)
    P = int(positive.sum())
    N = len(positive) - P
    if P == 0 or N == 0:
        return float("nan")
    tp, fp = _curve(scores, positive)
    tpr, fpr = np.r_[0.0, tp / P], np.r_[0.0, fp / N]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))


def _macro(v):
    keep = ~np.isnan(v)
    return float(v[keep].mean()) if keep.any() else float("nan")


def rank_from_scores(probs, labels, K):
    """probs (K, n) of one head, labels (n) (-1 = no label: the row is dropped) -> the dictionary of scores.rank_scores.
    A labelled row whose own-class score is not finite makes everything NaN."""
    probs, labels = np.asarray(probs, dtype=np.float64), np.asarray(labels)
    keep = (labels >= 0) & (labels < K)
    probs, labels = probs[:, keep], labels[keep]
    ap, auc = np.full(K, np.nan), np.full(K, np.nan)
    own = probs[labels, np.arange(labels.shape[0])] if labels.shape[0] else np.zeros(0)
    if not np.isfinite(own).all():
        return {"ap": ap, "roc_auc": auc, "ap_macro": float("nan"), "roc_auc_macro": float("nan")}
    for k in range(K):
        ap[k] = average_precision(probs[k], labels == k)
        auc[k] = roc_auc(probs[k], labels == k)
    return {"ap": ap, "roc_auc": auc, "ap_macro": _macro(ap), "roc_auc_macro": _macro(auc)}


#: the ranking score names per task (the reference's `auroc` is macro average precision: models/mimic.py:162-180)
NAMES = {"mimic": {"auroc": "ap_macro"}, "avmnist": {"ap_macro": "ap_macro", "roc_auc_macro": "roc_auc_macro"}}


def task(task_name, probs, labels, K, head_names):
    """probs (nheads, K, n): the task's names, the last head plain, the others with `_<modality>`."""
    out = {}
    last = len(head_names) - 1
    for h in [last] + list(range(last)):
        s = rank_from_scores(probs[h], labels, K)
        for name, key in NAMES[task_name].items():
            out[name + ("" if h == last else "_" + head_names[h])] = s[key]
    return out


def softmax64(logits):
    """Softmax over the last axis in float64 of (float32) logits."""
    x = np.asarray(logits).astype(np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
