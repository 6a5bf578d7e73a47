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

No torch, no GPU: importable anywhere.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

#: score names per task, for the fusion head, in the order of the reference's setup_scores dictionaries.  AV-MNIST: the four of
#: AVMnistMixerMultiLoss (models/avmnist.py:366-380) then the three micro scores its single-loss variant adds (:56-78).
#: MIMIC's `auroc` (a torchmetrics.AveragePrecision over ranked probabilities) is not a function of counts: not built.
TASK_SCORES: Dict[str, Tuple[str, ...]] = {
    "avmnist": ("acc", "f1m", "prec_m", "rec_m", "f1mi", "prec_mi", "rec_mi"),
    "mimic": ("f1_micro", "acc", "precision_micro", "recall_micro"),
    "mmimdb": ("f1w", "f1m"),
}
TASK_KIND = {"avmnist": "multiclass", "mimic": "multiclass", "mmimdb": "multilabel"}


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
