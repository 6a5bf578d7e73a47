"""CPU-side checks (-m "not gpu") of the scores: the derived numbers of m2_mixer_amd/scores.py against the numpy restatement
(tests/scores_ref.py) on hand-built count tables, against scikit-learn where it is installed and the definitions coincide, the
reference's key names per task, and the two new entry points in the header, the binding and the built library.

Both sides of every comparison are float64 arithmetic on the same integers in a different order: 1e-12 absolute is the bound
that follows from that (a handful of roundings of numbers <= 1), not a tuned tolerance.
"""
import os
import re

import numpy as np
import pytest

import scores_ref as R

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _S():
    from m2_mixer_amd import scores
    return scores


def _rows(seed, n, K, drop=()):
    """n random (pred, label) rows over K classes, 60 % of them correct; classes in `drop` occur in neither."""
    rng = np.random.default_rng(seed)
    keep = np.array([k for k in range(K) if k not in drop])
    labels = keep[rng.integers(0, len(keep), size=n)]
    preds = np.where(rng.random(n) < 0.6, labels, keep[rng.integers(0, len(keep), size=n)])
    return preds, labels


def _multiclass_cases():
    K = 10
    cases = {}
    p, l = _rows(1, 500, K)
    assert set(l.tolist()) == set(range(K))
    cases["all_present"] = (p, l, K)
    cases["class_9_absent"] = (*_rows(2, 500, K, drop=(9,)), K)
    p, l = _rows(3, 500, K, drop=(4,))
    p = p.copy()
    p[:17] = 4                                         # class 4: predicted 17 times, never true
    cases["predicted_never_true"] = (p, l, K)
    cases["empty"] = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), K)
    p, l = _rows(4, 64, 2)
    cases["binary"] = (p, l, 2)
    return cases


def _multilabel_cases():
    rng = np.random.default_rng(11)
    B, K = 300, 23
    targets = (rng.random((B, K)) < 0.15).astype(np.float32)
    preds = np.where(rng.random((B, K)) < 0.8, targets, (rng.random((B, K)) < 0.2)).astype(np.int32)
    targets[:, 5] = 0
    preds[:, 5] = 0                                    # label 5: never positive, never predicted
    preds[:, 7] = 0                                    # label 7: never predicted
    assert targets[:, 7].sum() > 0
    return {"mixed": (preds, targets, K), "empty": (np.zeros((0, K), np.int32), np.zeros((0, K), np.float32), K),
            "single_label": (preds[:, :1].copy(), targets[:, :1].copy(), 1)}


@pytest.mark.parametrize("name", list(_multiclass_cases()))
def test_multiclass_scores_equal_the_numpy_restatement(name):
    preds, labels, K = _multiclass_cases()[name]
    cm, skipped = R.confusion_matrix(preds, labels, K)
    assert skipped == 0 and cm.sum() == len(labels)
    got, want = _S().multiclass_scores(cm), R.multiclass(cm)
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (name, k, got[k], want[k])
        assert 0.0 <= got[k] <= 1.0
    if name == "empty":
        assert all(v == 0.0 for v in got.values())
    if name == "class_9_absent":
        # the absent class is left out of the macro mean: 9 classes, not 10 (scores.macro_class_weights)
        tp, fp, fn = _S().confusion_to_tp_fp_fn(cm)
        f1 = [2 * t / (2 * t + p + n) for t, p, n in zip(tp[:9], fp[:9], fn[:9])]
        assert abs(got["f1_macro"] - sum(f1) / 9) <= TOL
        assert _S().macro_class_weights(tp, fp, fn, multilabel=False).tolist() == [1.0] * 9 + [0.0]
    if name == "predicted_never_true":
        # class 4 has fp > 0: it stays in the macro mean with precision = recall = F1 = 0
        tp, fp, fn = _S().confusion_to_tp_fp_fn(cm)
        assert tp[4] == 0 and fp[4] == 17 and fn[4] == 0
        assert _S().macro_class_weights(tp, fp, fn, multilabel=False).tolist() == [1.0] * 10


@pytest.mark.parametrize("name", list(_multilabel_cases()))
def test_multilabel_scores_equal_the_numpy_restatement(name):
    preds, targets, K = _multilabel_cases()[name]
    table = R.multilabel_table(preds, targets, K)
    assert table.sum() == preds.size
    got, want = _S().multilabel_scores(table), R.multilabel(table)
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (name, k, got[k], want[k])
    if name == "empty":
        assert all(v == 0.0 for v in got.values())
    if name == "mixed":
        assert _S().macro_class_weights(table[:, 0], table[:, 1], table[:, 2], multilabel=True).tolist() == [1.0] * K


@pytest.mark.parametrize("name", ["all_present", "predicted_never_true", "binary"])
def test_multiclass_scores_equal_scikit_learn_where_the_definitions_agree(name):
    """Every class occurs among the labels or the predictions: the macro rule for an absent class does not come into play."""
    M = pytest.importorskip("sklearn.metrics")
    preds, labels, K = _multiclass_cases()[name]
    got = _S().multiclass_scores(R.confusion_matrix(preds, labels, K)[0])
    kw = dict(labels=list(range(K)), zero_division=0)
    want = {"acc": M.accuracy_score(labels, preds)}
    for avg in ("micro", "macro", "weighted"):
        want["prec_" + avg] = M.precision_score(labels, preds, average=avg, **kw)
        want["rec_" + avg] = M.recall_score(labels, preds, average=avg, **kw)
        want["f1_" + avg] = M.f1_score(labels, preds, average=avg, **kw)
    for k, v in want.items():
        assert abs(got[k] - float(v)) <= TOL, (name, k, got[k], v)


def test_multilabel_scores_equal_scikit_learn():
    M = pytest.importorskip("sklearn.metrics")
    preds, targets, K = _multilabel_cases()["mixed"]
    got = _S().multilabel_scores(R.multilabel_table(preds, targets, K))
    y, p = (targets >= 0.5).astype(int), (preds != 0).astype(int)
    for avg in ("micro", "macro", "weighted"):
        for name, fn in (("prec", M.precision_score), ("rec", M.recall_score), ("f1", M.f1_score)):
            want = float(fn(y, p, average=avg, zero_division=0))
            assert abs(got[f"{name}_{avg}"] - want) <= TOL, (name, avg, got[f"{name}_{avg}"], want)


# keys of the reference's setup_scores dictionaries (models/avmnist.py:56-78 and :366-380, models/mimic.py:162-180 without
# `auroc`, models/mmimdb.py:184-190)
REFERENCE_KEYS = {
    "avmnist": ["acc", "f1m", "prec_m", "rec_m", "f1mi", "prec_mi", "rec_mi"],
    "mimic": ["f1_micro", "acc", "precision_micro", "recall_micro"],
    "mmimdb": ["f1w", "f1m"],
}
HEADS = {"avmnist": ("image", "audio", "fusion"), "mimic": ("static", "time", "fusion"), "mmimdb": ("image", "text", "fusion")}


@pytest.mark.parametrize("task", list(REFERENCE_KEYS))
def test_task_scores_carry_the_reference_names(task):
    S = _S()
    assert list(S.TASK_SCORES[task]) == REFERENCE_KEYS[task]
    heads = HEADS[task]
    if task == "mmimdb":
        preds, targets, K = _multilabel_cases()["mixed"]
        counts = np.stack([R.multilabel_table(np.roll(preds, h, axis=0), targets, K) for h in range(3)])
    else:
        K = 10 if task == "avmnist" else 6
        counts = np.stack([R.confusion_matrix(*_rows(20 + h, 200, K), K)[0] for h in range(3)])
    got = S.task_scores(task, counts, heads)
    assert list(got)[:len(REFERENCE_KEYS[task])] == REFERENCE_KEYS[task]          # the fusion head: plain names, first
    want_keys = set(REFERENCE_KEYS[task]) | {f"{k}_{m}" for k in REFERENCE_KEYS[task] for m in heads[:2]}
    assert set(got) == want_keys
    want = R.task(task, counts, heads)
    assert set(want) == want_keys
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (task, k)
    # the plain names are the LAST head's
    one = (S.multilabel_scores if task == "mmimdb" else S.multiclass_scores)(counts[2])
    assert got[REFERENCE_KEYS[task][0]] == one[S._NAME_MAP[REFERENCE_KEYS[task][0]]]


def test_header_binding_and_library_carry_the_two_entry_points():
    from m2_mixer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    for name in ("m2m_scores_multiclass", "m2m_scores_multilabel"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/m2mixer.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define M2M_SCORES_MAX_CLASSES (\d+)", hdr).group(1)) == _lib.SCORES_MAX_CLASSES == 64
    assert int(re.search(r"#define M2M_SCORES_MAX_LABELS (\d+)", hdr).group(1)) == _lib.SCORES_MAX_LABELS == 128
    assert _lib.lib().m2m_abi_version() == 18          # new entry points only


def test_engines_and_modules_take_scores_defaulting_to_off():
    import inspect
    from m2_mixer_amd import engine as E, models as MD
    for cls in (E.AVMnistEngine, E.MimicEngine, E.MMIMDBEngine):
        assert inspect.signature(cls.__init__).parameters["scores"].default is False
        assert inspect.signature(cls.evaluate).parameters["scores"].default is None
    for fn in (MD._MultiLossModule.bind_engine, MD._MultiLossModule.to_engine):
        assert inspect.signature(fn).parameters["scores"].default is False
    for hook in ("training_epoch_end", "validation_epoch_end", "test_epoch_end"):
        assert inspect.signature(getattr(MD._MultiLossModule, hook)).parameters["outputs"].default is None
