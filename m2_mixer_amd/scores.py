"""Accuracy, precision, recall and F1 from integer count tables: host arithmetic in float64.

The reference keeps torchmetrics objects per task module (setup_scores: models/avmnist.py:366-380, models/mimic.py:162-180,
models/mmimdb.py:184-190) and logs their compute() at every epoch end (modules/train_test_module.py:86-151).  Here the steps
only add their counts into a device table (csrc/scores.hip, engine.ScoreTable); this module turns a table into the reference's
numbers, under the reference's names.

Definitions.  Per class k: tp, fp, fn; precision tp / (tp + fp), recall tp / (tp + fn),
F1 2 tp / (2 tp + fp + fn); a zero denominator gives 0.  micro: the same formulas on the sums over the classes (multiclass
accuracy: sum(tp) / N).  weighted: per-class scores weighted by the support tp + fn.  macro: see macro_class_weights -- the one
rule that differs between libraries.  This follows torchmetrics 0.11's `_adjust_weights_safe_divide` AS REMEMBERED: that
package is not a dependency of this project and the rule is not pinned against it (tests pin it against scikit-learn where the
two definitions coincide, and against a numpy restatement everywhere).

Ranking scores (MIMIC's `auroc` = macro average precision, ROC-AUC) are functions of four integers per sample, produced on the
device from a buffer of appended softmax rows (csrc/rank.hip, engine.RankBuffer): rank_scores / task_rank_scores below.

No torch, no GPU: importable anywhere.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

#: score names per task, for the fusion head, in the order of the reference's setup_scores dictionaries.  AV-MNIST: the four of
#: AVMnistMixerMultiLoss (models/avmnist.py:366-380) then the three micro scores its single-loss variant adds (:56-78).
#: MIMIC's `auroc` (a torchmetrics.AveragePrecision over ranked probabilities) is no function of THESE tables: it comes from the
#: ranking buffer's per-row counts (RANK_SCORES, rank_scores below).
TASK_SCORES: Dict[str, Tuple[str, ...]] = {
    "avmnist": ("acc", "f1m", "prec_m", "rec_m", "f1mi", "prec_mi", "rec_mi"),
    "mimic": ("f1_micro", "acc", "precision_micro", "recall_micro"),
    "mmimdb": ("f1w", "f1m"),
}
TASK_KIND = {"avmnist": "multiclass", "mimic": "multiclass", "mmimdb": "multilabel"}
#: ranking scores per task, for the fusion head (engine.RankBuffer, csrc/rank.hip).  MIMIC's `auroc` IS macro average precision:
#: the reference builds torchmetrics.AveragePrecision under that name (models/mimic.py:162-180); the name is kept.  ROC-AUC is
#: available on MIMIC too, as `roc_auc_macro` (task_rank_scores(..., names=...)).  Multilabel ranking (MM-IMDb) is not built.
RANK_SCORES: Dict[str, Tuple[str, ...]] = {"mimic": ("auroc",), "avmnist": ("ap_macro", "roc_auc_macro")}


def safe_divide(num, den):
    """num / den in float64; 0 where den == 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.zeros(np.broadcast(num, den).shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def confusion_to_tp_fp_fn(cm) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(K, K) confusion matrix [label][pred] -> per-class tp (diagonal), fp (column sum - tp), fn (row sum - tp)."""
    cm = np.asarray(cm, dtype=np.int64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"confusion matrix must be (K, K), got {cm.shape}")
    tp = np.diag(cm).copy()
    return tp, cm.sum(axis=0) - tp, cm.sum(axis=1) - tp


def macro_class_weights(tp, fp, fn, multilabel: bool) -> np.ndarray:
    """Which classes a macro average is taken over (1 / 0 per class).
    multilabel: all K labels.  multiclass: the classes with tp + fp + fn > 0 -- a class that occurs neither among the labels nor
    among the predictions is left out instead of entering with a score of 0.  (scikit-learn averages over all K in both cases:
    the two agree whenever every class occurs.)  The rule is torchmetrics 0.11's as remembered, unpinned: see the module text."""
    tp, fp, fn = (np.asarray(a, dtype=np.int64) for a in (tp, fp, fn))
    if multilabel:
        return np.ones(tp.shape, dtype=np.float64)
    return ((tp + fp + fn) > 0).astype(np.float64)


def _averages(tp, fp, fn, multilabel: bool) -> Dict[str, float]:
    tp, fp, fn = (np.asarray(a, dtype=np.int64) for a in (tp, fp, fn))
    per = {"prec": safe_divide(tp, tp + fp), "rec": safe_divide(tp, tp + fn), "f1": safe_divide(2 * tp, 2 * tp + fp + fn)}
    stp, sfp, sfn = int(tp.sum()), int(fp.sum()), int(fn.sum())
    micro = {"prec": safe_divide(stp, stp + sfp), "rec": safe_divide(stp, stp + sfn), "f1": safe_divide(2 * stp, 2 * stp + sfp + sfn)}
    wm = macro_class_weights(tp, fp, fn, multilabel)
    ww = (tp + fn).astype(np.float64)
    out = {}
    for name, v in per.items():
        out[name + "_micro"] = float(micro[name])
        out[name + "_macro"] = float(safe_divide((v * wm).sum(), wm.sum()))
        out[name + "_weighted"] = float(safe_divide((v * ww).sum(), ww.sum()))
    return out


def multiclass_scores(cm) -> Dict[str, float]:
    """acc and {prec, rec, f1}_{micro, macro, weighted} of a (K, K) confusion matrix [label][pred]."""
    tp, fp, fn = confusion_to_tp_fp_fn(cm)
    out = _averages(tp, fp, fn, multilabel=False)
    out["acc"] = float(safe_divide(int(tp.sum()), int(np.asarray(cm, dtype=np.int64).sum())))
    return out


def multilabel_scores(table) -> Dict[str, float]:
    """{prec, rec, f1}_{micro, macro, weighted} of a (K, 4) table of tp, fp, fn, tn per label."""
    t = np.asarray(table, dtype=np.int64)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError(f"multilabel table must be (K, 4), got {t.shape}")
    return _averages(t[:, 0], t[:, 1], t[:, 2], multilabel=True)


# reference name -> key of multiclass_scores / multilabel_scores
_NAME_MAP = {
    "acc": "acc", "f1m": "f1_macro", "prec_m": "prec_macro", "rec_m": "rec_macro", "f1mi": "f1_micro", "prec_mi": "prec_micro",
    "rec_mi": "rec_micro", "f1_micro": "f1_micro", "precision_micro": "prec_micro", "recall_micro": "rec_micro", "f1w": "f1_weighted",
}


def task_scores(task: str, counts, head_names: Sequence[str]) -> Dict[str, float]:
    """The reference's score names for `task` ("avmnist", "mimic", "mmimdb") from the per-head count tables `counts`
    ((nheads, K, K) confusion matrices or (nheads, K, 4) tp / fp / fn / tn): the LAST head is the fusion head and takes the plain
    names (`acc`, `f1m`, ...), the other heads the same names with `_<modality>` appended."""
    names = TASK_SCORES[task]
    counts = np.asarray(counts, dtype=np.int64)
    if counts.shape[0] != len(head_names):
        raise ValueError(f"{counts.shape[0]} tables for {len(head_names)} heads")
    fn = multilabel_scores if TASK_KIND[task] == "multilabel" else multiclass_scores
    out: Dict[str, float] = {}
    order = [len(head_names) - 1] + list(range(len(head_names) - 1))
    for h in order:
        s = fn(counts[h])
        suffix = "" if h == len(head_names) - 1 else "_" + head_names[h]
        for n in names:
            out[n + suffix] = s[_NAME_MAP[n]]
    return out


# ---- ranking scores: average precision and ROC-AUC from per-row counts -----------------------------------------------------------
def rank_scores(counts, labels, K: int) -> Dict[str, object]:
    """Per-class and macro average precision and ROC-AUC (one-vs-rest) of ONE head from its per-row counts.

    counts (n, 4) integers {n_ge, p_ge, n_gt, p_gt} and labels (n) as m2m_rank_counts / engine.RankBuffer.counts() give them: for
    row i of class c = labels[i] with score s_i = p_i[c], n_ge / p_ge = the rows / the class-c rows whose class-c score is >= s_i
    (row i included), n_gt / p_gt the same with >; rows with label -1 carry zeros and were invisible to the others.  With
    P_c = the rows of class c, N_c = the other labelled rows:

      AP_c  = (1 / P_c) sum_{i: y_i = c} p_ge(i) / n_ge(i)
      AUC_c = (1 / (P_c N_c)) sum_{i: y_i = c} [ N_c - (n_ge - p_ge) + ((n_ge - n_gt) - (p_ge - p_gt)) / 2 ]

    Tied scores form one threshold, as in torchmetrics and scikit-learn: every positive of a tie group sees the whole group in
    its >= counts (AP: the precision at the group's threshold), and a positive tied with a negative scores 1/2 (AUC).
    Returns {"ap": (K,), "roc_auc": (K,), "ap_macro": float, "roc_auc_macro": float}; a class without positives is NaN in both
    arrays, a class without negatives NaN in roc_auc.  Macro: the mean over the classes that are not NaN -- a class without
    positives is left out of both means, one without negatives also out of roc_auc_macro; no class left: NaN.  Like
    macro_class_weights this is torchmetrics' rule AS REMEMBERED and unpinned (scikit-learn agrees wherever every class has a
    positive and a negative, which is what the tests pin).
    A labelled row with n_ge == 0 did not count itself: its score is not finite (NaN compares false).  Everything is NaN then."""
    c = np.asarray(counts).astype(np.int64).reshape(-1, 4)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    if c.shape[0] != y.shape[0]:
        raise ValueError(f"{c.shape[0]} count rows for {y.shape[0]} labels")
    if ((y < -1) | (y >= K)).any():
        raise ValueError(f"labels must lie in [0, {K}) or be -1 (skipped)")
    nan = float("nan")
    ap, auc = np.full(K, nan), np.full(K, nan)
    valid = y >= 0
    if (c[valid, 0] == 0).any():
        return {"ap": ap, "roc_auc": auc, "ap_macro": nan, "roc_auc_macro": nan}
    nv = int(valid.sum())
    n_ge, p_ge, n_gt, p_gt = (c[:, k].astype(np.float64) for k in range(4))
    for k in range(int(K)):
        rows = y == k
        P = int(rows.sum())
        N = nv - P
        if P == 0:
            continue
        ap[k] = float((p_ge[rows] / n_ge[rows]).sum()) / P
        if N > 0:
            wins = N - (n_ge[rows] - p_ge[rows]) + 0.5 * ((n_ge[rows] - n_gt[rows]) - (p_ge[rows] - p_gt[rows]))
            auc[k] = float(wins.sum()) / (float(P) * float(N))

    def macro(v):
        keep = ~np.isnan(v)
        return float(v[keep].mean()) if keep.any() else nan

    return {"ap": ap, "roc_auc": auc, "ap_macro": macro(ap), "roc_auc_macro": macro(auc)}


# reference name -> key of rank_scores
_RANK_NAME_MAP = {"auroc": "ap_macro", "ap_macro": "ap_macro", "roc_auc_macro": "roc_auc_macro"}


def task_rank_scores(task: str, counts, labels, K: int, head_names: Sequence[str], names: Sequence[str] = None) -> Dict[str, float]:
    """RANK_SCORES[task] (or `names`, any of auroc / ap_macro / roc_auc_macro) from the per-head row counts (nheads, n, 4) and the
    n row labels: the LAST head is the fusion head and takes the plain names, the other heads `_<modality>`, as task_scores."""
    names = RANK_SCORES[task] if names is None else tuple(names)
    counts = np.asarray(counts)
    if counts.ndim != 3 or counts.shape[0] != len(head_names) or counts.shape[2] != 4:
        raise ValueError(f"counts must be ({len(head_names)}, n, 4), got {counts.shape}")
    out: Dict[str, float] = {}
    last = len(head_names) - 1
    for h in [last] + list(range(last)):
        s = rank_scores(counts[h], labels, K)
        suffix = "" if h == last else "_" + head_names[h]
        for n in names:
            out[n + suffix] = s[_RANK_NAME_MAP[n]]
    return out
