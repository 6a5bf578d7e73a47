"""Reference side of the score tests: plain-loop count tables and a float64 numpy restatement of the derived numbers
(DESIGN.md section 10), written independently of m2_mixer_amd/scores.py -- per-class arrays, np.mean / np.average instead of
weight vectors -- so that the two agree only if both follow the definitions.

Definitions: per class tp, fp, fn; precision tp / (tp + fp), recall tp / (tp + fn), F1 2 tp / (2 tp + fp + fn), 0 where the
denominator is 0.  micro: on the sums.  macro multiclass: mean over the classes with tp + fp + fn > 0.  macro multilabel: mean
over all labels.  weighted: by the support tp + fn.  accuracy (multiclass): sum(tp) / N.
"""
import numpy as np


def confusion_matrix(preds, labels, K):
    """(K, K) int64 [label][pred] and the number of rows with a label or prediction outside [0, K)."""
    cm, skipped = np.zeros((K, K), dtype=np.int64), 0
    for p, l in zip(np.asarray(preds).tolist(), np.asarray(labels).tolist()):
        if 0 <= l < K and 0 <= p < K:
            cm[l][p] += 1
        else:
            skipped += 1
    return cm, skipped


def multilabel_table(preds, targets, K):
    """(K, 4) int64: tp, fp, fn, tn per label; preds (B, K) non-zero = predicted, targets (B, K) positive when >= 0.5."""
    t = np.zeros((K, 4), dtype=np.int64)
    preds, targets = np.asarray(preds), np.asarray(targets)
    for b in range(preds.shape[0]):
        for k in range(K):
            pos, hit = bool(targets[b][k] >= 0.5), bool(preds[b][k] != 0)
            t[k][(0 if hit else 2) if pos else (1 if hit else 3)] += 1
    return t


def _div(a, b):
    return float(a) / float(b) if b != 0 else 0.0


def _scores(tp, fp, fn, macro_over):
    K = len(tp)
    prec = np.array([_div(tp[k], tp[k] + fp[k]) for k in range(K)], dtype=np.float64)
    rec = np.array([_div(tp[k], tp[k] + fn[k]) for k in range(K)], dtype=np.float64)
    f1 = np.array([_div(2 * tp[k], 2 * tp[k] + fp[k] + fn[k]) for k in range(K)], dtype=np.float64)
    support = np.array([tp[k] + fn[k] for k in range(K)], dtype=np.float64)
    TP, FP, FN = int(sum(tp)), int(sum(fp)), int(sum(fn))
    out = {"prec_micro": _div(TP, TP + FP), "rec_micro": _div(TP, TP + FN), "f1_micro": _div(2 * TP, 2 * TP + FP + FN)}
    for name, v in (("prec", prec), ("rec", rec), ("f1", f1)):
        out[name + "_macro"] = float(np.mean(v[macro_over])) if len(macro_over) else 0.0
        out[name + "_weighted"] = float(np.average(v, weights=support)) if support.sum() > 0 else 0.0
    return out


def multiclass(cm):
    cm = np.asarray(cm, dtype=np.int64)
    K = cm.shape[0]
    tp = [int(cm[k][k]) for k in range(K)]
    fp = [int(cm[:, k].sum()) - tp[k] for k in range(K)]
    fn = [int(cm[k, :].sum()) - tp[k] for k in range(K)]
    out = _scores(tp, fp, fn, [k for k in range(K) if tp[k] + fp[k] + fn[k] > 0])
    out["acc"] = _div(sum(tp), int(cm.sum()))
    return out


def multilabel(table):
    t = np.asarray(table, dtype=np.int64)
    return _scores([int(x) for x in t[:, 0]], [int(x) for x in t[:, 1]], [int(x) for x in t[:, 2]], list(range(t.shape[0])))


# the reference's names (keys of its setup_scores dictionaries, `auroc` left out) -> key above
NAMES = {
    "avmnist": {"acc": "acc", "f1m": "f1_macro", "prec_m": "prec_macro", "rec_m": "rec_macro", "f1mi": "f1_micro",
                "prec_mi": "prec_micro", "rec_mi": "rec_micro"},
    "mimic": {"f1_micro": "f1_micro", "acc": "acc", "precision_micro": "prec_micro", "recall_micro": "rec_micro"},
    "mmimdb": {"f1w": "f1_weighted", "f1m": "f1_macro"},
}


def task(task_name, counts, head_names, prefix=""):
    """{prefix + name (+ '_' + modality for the heads before the last)} from per-head tables."""
    fn = multilabel if task_name == "mmimdb" else multiclass
    out = {}
    for h, head in enumerate(head_names):
        s = fn(counts[h])
        suffix = "" if h == len(head_names) - 1 else "_" + head
        for name, key in NAMES[task_name].items():
            out[prefix + name + suffix] = s[key]
    return out
