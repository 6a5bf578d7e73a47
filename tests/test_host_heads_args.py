"""The one argument check of the heads' entry points (m2m_check_heads, csrc/heads.hip), on a machine without a GPU: a refusal
precedes every HIP call -- the losses' zero fill included -- so placeholder pointers suffice, and a call the check wrongly let
through would find no device instead of launching on them.  Every case returns -1 with a message, through the cross-entropy,
the BCE and the evidential entry alike: the NULLs that only m2m_heads_edl refused until the check became one, and the refusals
all three had."""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder pointers: only where no GPU can be launched on")

B, D, K, NH = 5, 32, 3, 2
P = 0x10000                        # a placeholder "device pointer": non-NULL, 16-byte aligned, never dereferenced
HEAD_FIELDS = ("w", "b")
CALL_POINTERS = ("labels", "logits", "losses", "preds")

# the refusals that the three entries did not share: each NULL, and d_pooled without a place for the weight gradients
NEW_REFUSALS = [f"NULL {f}" for f in HEAD_FIELDS + CALL_POINTERS] + ["d_pooled without g_w", "d_pooled without g_b",
                                                                    "d_pooled without g_w, g_b and g_part"]
# the refusals all of them had (m2m_heads_edl's own list, and what tests/test_gpu_heads.py refuses on the GPU)
OLD_REFUSALS = ["NULL heads", "no heads", "five heads", "K=1", "K=33", "D=48", "B=0", "neither pooled nor tokens", "tokens unaligned",
                "ntok=0", "stride below ntok*D", "stride not a multiple of 4", "g_part K23 D64"]
EDL_ONLY = ["NULL uncertainty", "NULL combined", "risk=2", "kl_out without kl_coef"]
BCE_ONLY = ["NULL pos_weight", "g_part on BCE"]


def refused(loss, what):
    from m2_mixer_amd import _lib as L
    b, d, k, nh = B, D, K, NH
    call = dict(labels=P, logits=P, losses=P, preds=P, pos_weight=P, uncertainty=P, combined=P, kl_coef=0, kl_out=0)
    risk = L.EDL_MSE
    arr = (L.Head * 5)()
    for h in arr:
        h.pooled, h.w, h.b, h.g_w, h.g_b, h.d_pooled, h.weight = P, P, P, P, P, P, 1.0
    last = arr[NH - 1]                                  # the defect sits in the last head: every head is looked at
    if what.startswith("NULL ") and what[5:] in HEAD_FIELDS: setattr(last, what[5:], 0)
    elif what.startswith("NULL ") and what[5:] in call: call[what[5:]] = 0
    elif what == "d_pooled without g_w": last.g_w = 0
    elif what == "d_pooled without g_b": last.g_b = 0
    elif what == "d_pooled without g_w, g_b and g_part": last.g_w = last.g_b = 0
    elif what == "NULL heads": arr = None
    elif what == "no heads": nh = 0
    elif what == "five heads": nh = 5
    elif what == "K=1": k = 1
    elif what == "K=33": k = 33
    elif what == "D=48": d = 48
    elif what == "B=0": b = 0
    elif what == "neither pooled nor tokens": last.pooled = 0
    elif what == "tokens unaligned": last.tokens, last.ntok, last.tok_sample_stride = P + 4, 4, 4 * D
    elif what == "ntok=0": last.tokens, last.ntok, last.tok_sample_stride = P, 0, 4 * D
    elif what == "stride below ntok*D": last.tokens, last.ntok, last.tok_sample_stride = P, 4, 4 * D - 4
    elif what == "stride not a multiple of 4": last.tokens, last.ntok, last.tok_sample_stride = P, 4, 4 * D + 2
    elif what == "g_part K23 D64": last.g_part, k, d = P, 23, 64
    elif what == "g_part on BCE": last.g_part = P
    elif what == "risk=2": risk = 2
    elif what == "kl_out without kl_coef": call["kl_out"] = P
    else: raise AssertionError(what)
    lib = L.lib()
    if loss == "ce":
        rc = lib.m2m_heads_ce_w(arr, nh, call["labels"], b, d, k, call["logits"], call["losses"], call["preds"], 1, 0, 0)
    elif loss == "bce":
        rc = lib.m2m_heads_bce_w(arr, nh, call["labels"], call["pos_weight"], b, d, k, call["logits"], call["losses"], call["preds"], 1, 0, 0)
    else:
        rc = lib.m2m_heads_edl_risk(arr, nh, call["labels"], b, d, k, call["logits"], call["losses"], call["preds"], call["uncertainty"],
                                    call["combined"], 1, 0, risk, call["kl_coef"], call["kl_out"], 0)
    return rc, lib.m2m_last_error()


@pytest.mark.parametrize("what", NEW_REFUSALS + OLD_REFUSALS)
@pytest.mark.parametrize("loss", ["ce", "bce", "edl"])
def test_every_entry_refuses_what_any_of_them_refused(loss, what):
    rc, msg = refused(loss, what)
    assert rc == -1 and len(msg) > 0
    assert msg.startswith(b"heads_" + loss.encode())                      # the message names the call that was refused


@pytest.mark.parametrize("loss,what", [("edl", w) for w in EDL_ONLY] + [("bce", w) for w in BCE_ONLY])
def test_the_refusals_of_one_loss_alone(loss, what):
    rc, msg = refused(loss, what)
    assert rc == -1 and len(msg) > 0 and msg.startswith(b"heads_" + loss.encode())


def test_the_plain_entries_run_the_same_check():
    """m2m_heads_ce / _bce / m2m_heads_edl are the _w / _risk calls with the trailing arguments absent."""
    from m2_mixer_amd import _lib as L
    arr = (L.Head * 2)()
    for h in arr:
        h.pooled, h.w, h.g_w, h.g_b, h.d_pooled, h.weight = P, P, P, P, P, 1.0          # b is NULL
    lib = L.lib()
    assert lib.m2m_heads_ce(arr, NH, P, B, D, K, P, P, P, 1, 0) == -1 and lib.m2m_last_error().startswith(b"heads_ce")
    assert lib.m2m_heads_bce(arr, NH, P, P, B, D, K, P, P, P, 1, 0) == -1 and lib.m2m_last_error().startswith(b"heads_bce")
    assert lib.m2m_heads_edl(arr, NH, P, B, D, K, P, P, P, P, P, 1, 0, 0) == -1 and lib.m2m_last_error().startswith(b"heads_edl")
