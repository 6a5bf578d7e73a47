"""The epoch feed restated in numpy (csrc/feed.hip, include/m2mixer.h "epoch feed"): what one m2m_feed_gather launch leaves in the
slots and in `state`, and what one m2m_epoch_accumulate launch adds to the accumulators."""
import numpy as np

CURSOR, TICKET, ROWS, WRAPPED = 0, 1, 2, 3        # the uint32 words of `state`


def gather(sources, perm, state, B):
    """sources: arrays of n rows each; perm: n indices or None; state: the 4 words before the launch.
    -> (expected slot contents as raw bytes, one (B, row_bytes) uint8 array per source; the 4 words after the launch)."""
    cursor, n = int(state[CURSOR]), int(state[ROWS])
    at = [(cursor + r) % n for r in range(B)]
    idx = at if perm is None else [int(perm[a]) for a in at]
    slots = []
    for s in sources:
        rows = np.ascontiguousarray(s).reshape(s.shape[0], -1).view(np.uint8)
        slots.append(np.stack([rows[i] for i in idx]))
    after = np.array(state, dtype=np.uint32).copy()
    after[CURSOR] = (cursor + B) & 0xFFFFFFFF
    after[TICKET] = 0
    after[WRAPPED] = (int(state[WRAPPED]) + max(0, cursor + B - n)) & 0xFFFFFFFF
    return slots, after


def raw(a):
    """A (rows, ...) array as (rows, row_bytes) uint8."""
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def accumulate(sums, counts, losses, preds, labels, B):
    """One step added to (sums float64 (2 nloss), counts int64 (nheads + 2)); preds (nheads, B) or None (nheads = 0)."""
    losses = np.asarray(losses, dtype=np.float32).astype(np.float64)
    nloss = losses.shape[0]
    nheads = 0 if preds is None else preds.shape[0]
    sums, counts = sums.copy(), counts.copy()
    sums[:nloss] += losses
    sums[nloss:] += losses * float(B)
    for h in range(nheads):
        counts[h] += int((preds[h].astype(np.int64) == labels).sum())
    counts[nheads] += 1
    counts[nheads + 1] += B
    return sums, counts
