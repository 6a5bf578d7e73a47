"""The muted gather restated in numpy (csrc/feed.hip: m2m_feed_gather_muted): what one launch leaves in the slots, in `state` and
in `mute_state`.  Written on its own, not on top of feed_ref.gather, so that the two can be checked against each other."""
import numpy as np

STEP, PAST = 0, 1                                  # the uint32 words of `mute_state`


def gather_muted(sources, perm, state, B, codes, mute_state):
    """sources: arrays of n rows each; perm: n indices or None; state: the feed's 4 words; codes: the schedule (int array, may be
    empty); mute_state: the 2 words before the launch.
    -> (one (B, row_bytes) uint8 array per source, the 4 state words after, the 2 mute_state words after)."""
    cursor, n = int(state[0]), int(state[2])
    step = int(mute_state[STEP])
    code = int(codes[step]) if step < len(codes) else 0
    slots = []
    for s, src in enumerate(sources):
        rows = np.ascontiguousarray(src).reshape(src.shape[0], -1).view(np.uint8)
        if code == s + 1:
            slots.append(np.zeros((B, rows.shape[1]), dtype=np.uint8))
            continue
        out = np.empty((B, rows.shape[1]), dtype=np.uint8)
        for r in range(B):
            at = (cursor + r) % n
            out[r] = rows[at if perm is None else int(perm[at])]
        slots.append(out)
    after = np.array(state, dtype=np.uint32).copy()
    after[0] = (cursor + B) & 0xFFFFFFFF
    after[1] = 0
    after[3] = (int(state[3]) + max(0, cursor + B - n)) & 0xFFFFFFFF
    mute_after = np.array(mute_state, dtype=np.uint32).copy()
    mute_after[STEP] = (step + 1) & 0xFFFFFFFF
    if step >= len(codes):
        mute_after[PAST] += 1
    return slots, after, mute_after
