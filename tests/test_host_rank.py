"""CPU-side checks (-m "not gpu") of the ranking scores: scores.rank_scores on plain-loop counts (tests/rank_ref.py) against
scikit-learn where it is installed and the macro rules coincide, against the sort-based restatement everywhere, the names per
task, and the two entry points in the header, the binding and the built library.

Both sides of every comparison are float64 arithmetic on the same ranking in a different order (sums of at most n quotients
<= 1 divided by a count): 1e-12 absolute follows from that for the n <= 700 used here, it is not a tuned tolerance.
"""
import inspect
import os
import re

import numpy as np
import pytest

import rank_ref as R

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = {"avmnist": ("image", "audio", "fusion"), "mimic": ("static", "time", "fusion")}


def _S():
    from m2_mixer_amd import scores
    return scores


def _softmax_rows(rng, n, K, scale=2.0):
    return R.softmax64(rng.normal(size=(n, K)).astype(np.float32) * scale).T.copy()         # (K, n)


def _cases():
    """name -> (probs (K, n) float64, labels (n), K)."""
    out = {}
    rng = np.random.default_rng(11)
    n, K = 300, 6
    out["random"] = (_softmax_rows(rng, n, K), rng.integers(0, K, size=n), K)
    lab = rng.integers(0, 5, size=n)                                                        # class 5 never occurs
    out["class_without_positives"] = (_softmax_rows(rng, n, K), lab, K)
    out["class_with_only_positives"] = (_softmax_rows(rng, 40, 3), np.full(40, 1), 3)       # classes 0, 2 absent, class 1 universal
    p = _softmax_rows(rng, n, K)
    p[2, :] = 0.25                                                                          # an all-equal column
    out["all_equal_column"] = (p, rng.integers(0, K, size=n), K)
    levels = np.array([0.0, 0.125, 0.25, 0.5, 1.0])
    out["five_levels"] = (levels[rng.integers(0, 5, size=(K, 700))], rng.integers(0, K, size=700), K)
    out["n_1"] = (np.array([[0.3], [0.7]]), np.array([1]), 2)
    out["n_2_tied"] = (np.array([[0.5, 0.5], [0.5, 0.5]]), np.array([0, 1]), 2)
    lab = rng.integers(0, K, size=n)
    lab[::7] = -1                                                                           # rows without a label
    out["skipped_rows"] = (_softmax_rows(rng, n, K), lab, K)
    out["k_64"] = (_softmax_rows(rng, 200, 64), rng.permutation(200) % 64, 64)             # every class occurs
    return out


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= TOL))


@pytest.mark.parametrize("name", list(_cases()))
def test_rank_scores_equal_the_sort_based_restatement(name):
    probs, labels, K = _cases()[name]
    counts = R.rank_counts(probs, labels, K)
    assert np.array_equal(counts, R.rank_counts_fast(probs, labels, K))
    got, want = _S().rank_scores(counts, labels, K), R.rank_from_scores(probs, labels, K)
    assert set(got) == {"ap", "roc_auc", "ap_macro", "roc_auc_macro"}
    for k in want:
        assert _close(got[k], want[k]), (name, k, got[k], want[k])
    assert isinstance(got["ap_macro"], float) and isinstance(got["roc_auc_macro"], float)
    if name == "class_without_positives":
        assert np.isnan(got["ap"][5]) and np.isnan(got["roc_auc"][5]) and not np.isnan(got["ap"][:5]).any()
        assert abs(got["ap_macro"] - got["ap"][:5].mean()) <= TOL             # the class is left out, not averaged in as 0
    if name == "class_with_only_positives":
        assert got["ap"][1] == 1.0 and np.isnan(got["roc_auc"]).all() and got["ap_macro"] == 1.0 and np.isnan(got["roc_auc_macro"])
    if name == "n_1":
        assert counts.tolist() == [[1, 1, 0, 0]] and got["ap_macro"] == 1.0
    if name == "n_2_tied":
        assert got["ap"].tolist() == [0.5, 0.5] and got["roc_auc"].tolist() == [0.5, 0.5]
    if name == "skipped_rows":
        assert (counts[::7] == 0).all()
        keep = labels >= 0
        alone = _S().rank_scores(R.rank_counts(probs[:, keep], labels[keep], K), labels[keep], K)
        assert _close(got["ap"], alone["ap"]) and _close(got["roc_auc"], alone["roc_auc"])      # invisible to the others


@pytest.mark.parametrize("name", ["random", "all_equal_column", "five_levels", "k_64"])
def test_rank_scores_equal_scikit_learn_where_the_definitions_agree(name):
    """Every class has a positive and a negative: the macro rules of the two libraries coincide."""
    M = pytest.importorskip("sklearn.metrics")
    probs, labels, K = _cases()[name]
    assert all(0 < int((labels == k).sum()) < labels.shape[0] for k in range(K))
    got = _S().rank_scores(R.rank_counts_fast(probs, labels, K), labels, K)
    for k in range(K):
        y = (labels == k).astype(int)
        assert abs(got["ap"][k] - float(M.average_precision_score(y, probs[k]))) <= TOL, (name, k)
        assert abs(got["roc_auc"][k] - float(M.roc_auc_score(y, probs[k]))) <= TOL, (name, k)
    onehot = (labels[:, None] == np.arange(K)[None, :]).astype(int)
    assert abs(got["ap_macro"] - float(M.average_precision_score(onehot, probs.T, average="macro"))) <= TOL
    assert abs(got["roc_auc_macro"] - float(M.roc_auc_score(onehot, probs.T, average="macro"))) <= TOL


def test_a_labelled_row_that_does_not_count_itself_gives_nan():
    """n_ge == 0 on a labelled row: its score compared false with itself, i.e. it is not finite."""
    S = _S()
    probs, labels, K = _cases()["random"]
    probs = probs.copy()
    probs[labels[17], 17] = np.nan
    counts = R.rank_counts(probs, labels, K)
    assert counts[17].tolist() == [0, 0, 0, 0]
    got = S.rank_scores(counts, labels, K)
    assert np.isnan(got["ap"]).all() and np.isnan(got["roc_auc"]).all() and np.isnan(got["ap_macro"]) and np.isnan(got["roc_auc_macro"])
    assert _close(got["ap"], R.rank_from_scores(probs, labels, K)["ap"])
    # zeros on a row WITHOUT a label are the normal case
    labels = labels.copy()
    labels[17] = -1
    assert not np.isnan(S.rank_scores(R.rank_counts(probs, labels, K), labels, K)["ap_macro"])
    with pytest.raises(ValueError):
        S.rank_scores(counts, np.full(labels.shape, K), K)
    with pytest.raises(ValueError):
        S.rank_scores(counts[:-1], labels, K)


@pytest.mark.parametrize("task", ["mimic", "avmnist"])
def test_task_rank_scores_carry_the_names(task):
    S = _S()
    assert S.RANK_SCORES == {"mimic": ("auroc",), "avmnist": ("ap_macro", "roc_auc_macro")}
    # the count-table names are what they were
    assert S.TASK_SCORES == {"avmnist": ("acc", "f1m", "prec_m", "rec_m", "f1mi", "prec_mi", "rec_mi"),
                             "mimic": ("f1_micro", "acc", "precision_micro", "recall_micro"), "mmimdb": ("f1w", "f1m")}
    heads, K, n = HEADS[task], 6, 150
    rng = np.random.default_rng(3)
    probs = np.stack([_softmax_rows(rng, n, K) for _ in heads])
    labels = rng.integers(0, K, size=n)
    counts = np.stack([R.rank_counts_fast(probs[h], labels, K) for h in range(3)])
    got = S.task_rank_scores(task, counts, labels, K, heads)
    names = S.RANK_SCORES[task]
    assert list(got)[:len(names)] == list(names)                                         # the fusion head: plain names, first
    assert set(got) == set(names) | {f"{k}_{m}" for k in names for m in heads[:2]}
    want = R.task(task, probs, labels, K, heads)
    assert set(want) == set(got)
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (task, k)
    fusion = S.rank_scores(counts[2], labels, K)
    assert got[names[0]] == fusion["ap_macro"]                                           # `auroc` IS macro average precision
    # ROC-AUC on MIMIC, under its own name
    both = S.task_rank_scores(task, counts, labels, K, heads, names=("auroc", "roc_auc_macro"))
    assert both["roc_auc_macro"] == fusion["roc_auc_macro"] and both["auroc"] == fusion["ap_macro"]
    assert set(both) == {"auroc", "roc_auc_macro"} | {f"{k}_{m}" for k in ("auroc", "roc_auc_macro") for m in heads[:2]}
    with pytest.raises(ValueError):
        S.task_rank_scores(task, counts[:2], labels, K, heads)


def test_header_binding_and_library_carry_the_rank_entry_points():
    from m2_mixer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    for name in ("m2m_rank_append", "m2m_rank_counts"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/m2mixer.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define M2M_RANK_STATE_WORDS (\d+)", hdr).group(1)) == _lib.RANK_STATE_WORDS == 4
    assert len(_lib.SIGNATURES["m2m_rank_append"][1]) == 10 and len(_lib.SIGNATURES["m2m_rank_counts"][1]) == 8
    assert "models/mimic.py:126-128" in hdr and "models/mimic.py:162-180" in hdr
    assert _lib.lib().m2m_abi_version() == 18 == _lib.ABI_VERSION          # new entry points only


def test_rank_scores_default_to_off_everywhere():
    from m2_mixer_amd import engine as E, models as MD
    for cls in (E.AVMnistEngine, E.MimicEngine, E.MMIMDBEngine):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["rank_scores"].default is False and sig["rank_capacity"].default == 65536
        assert inspect.signature(cls.evaluate).parameters["rank"].default is None
    for fn in (MD._MultiLossModule.bind_engine, MD._MultiLossModule.to_engine):
        sig = inspect.signature(fn).parameters
        assert sig["rank_scores"].default is False and sig["rank_capacity"].default == 65536
    assert "mmimdb" not in _S().RANK_SCORES


def test_mmimdb_engine_refuses_rank_scores():
    """Multilabel ranking is not built: refused by name before anything is allocated (no GPU needed to be told so)."""
    import gen_util as G
    from m2_mixer_amd.engine import MMIMDBEngine
    with pytest.raises(RuntimeError, match="multilabel ranking is not built"):
        MMIMDBEngine(G.MMIMDB, 8, device="cpu", rank_scores=True)
