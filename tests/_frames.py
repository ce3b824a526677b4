"""How each slot of the 40-double reduction record scales with the clouds' unit (shared by the frame tests).

Read off acc_pair (icp-symm_amd/csrc/kernels_pass.hip) and include/symmicp.h.  PAPER and QUIRKS rows: v = (m, n) with
m = (p + q) x n a length (~ s) and n = np + nq a pure number (~ 1), c = (p - q) . n a length.  Clouds scaled by s scale
slot k of the record by exactly s ** dims[k] when s is a power of two (fp64 sums of exactly scaled terms)."""
import numpy as np

NSUM = 40


def record_dims(p2p=False):
    d = np.zeros(NSUM, np.int64)
    if p2p:
        d[0:9] = 2                          # sum p q^T
    else:
        k = 0
        for r in range(6):
            for c in range(r, 6):
                d[k] = (r < 3) + (c < 3)    # m.m ~ s^2, m.n ~ s, n.n ~ 1
                k += 1
        d[21:24] = 2                        # sum m c
        d[24:27] = 1                        # sum n c
        d[35] = 2                           # sum c^2
    d[27:33] = 1                            # sum p, sum q (about the pivot)
    d[33] = 1                               # sum |p - q|
    d[34] = 0                               # pairs (robust: sum of weights)
    d[36] = 2                               # sum |p - q|^2
    return d                                # [37] pair count with a robust loss, [38..39] zero: 0


def scale_record(S, s, p2p=False):
    """the record of the same pairs in clouds scaled by the power of two s"""
    return np.asarray(S, np.float64) * np.float64(s) ** record_dims(p2p)
