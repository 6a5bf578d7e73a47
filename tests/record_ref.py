"""The prediction record's append restated in numpy (csrc/record.hip, include/m2mixer.h "prediction record"): what one
m2m_record_append launch leaves in the destinations and in `state`."""
import numpy as np

ROWS, RESERVED1, RESERVED2, DROPPED = 0, 1, 2, 3        # the uint32 words of `state`


def raw(a):
    """A (rows, ...) array as (rows, row_bytes) uint8."""
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def append(dsts, srcs, state, capacity):
    """dsts: (capacity or more, row_bytes) uint8 arrays, one per source, as they are before the launch; srcs: (B, row_bytes) uint8
    arrays; state: the 4 words before the launch.  -> (the destinations after the launch, the 4 words after the launch).  Row r of
    a source lands in row state[ROWS] + r where that is below `capacity`; every other row is dropped and counted."""
    cursor, B = int(state[ROWS]), int(srcs[0].shape[0])
    keep = max(0, min(B, capacity - cursor))
    out = []
    for d, s in zip(dsts, srcs):
        d = d.copy()
        d[cursor:cursor + keep] = s[:keep]
        out.append(d)
    after = np.array(state, dtype=np.uint32).copy()
    after[ROWS] = (cursor + B) & 0xFFFFFFFF
    after[DROPPED] = (int(state[DROPPED]) + B - keep) & 0xFFFFFFFF
    return out, after
