"""A numpy restatement of mgcn_sample_rows's definition (include/mgcn.h): the
yardstick of tests/test_sample_host.py and tests/test_gpu_sample.py.

key(e) is output word 0, all 32 bits, of the Philox4x32-10 call that
mgcn_edge_noise makes for head 0 of COO edge e (philox_ref).  Among the
candidates of one destination row, ordered by (key(e), e) ascending, the first
min(fanout, #candidates) are kept; with keep_loops a self loop is no candidate,
it is kept and not counted; a row with rows[dst] false keeps nothing."""
import numpy as np

import philox_ref as pr


def keys(seed, offset, nnz):
    """uint32 [nnz]: key(e) of COO edges e = 0 .. nnz - 1."""
    ctr = np.empty((nnz, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nnz, dtype=np.uint32)
    ctr[:, 1] = 0
    ctr[:, 2] = offset & 0xFFFFFFFF
    ctr[:, 3] = (offset >> 32) & 0xFFFFFFFF
    return pr.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[:, 0]


def sample_keep(src, dst, n, fanout, seed, offset, keep_loops=True, rows=None):
    """bool [nnz] in COO order: one lexsort by (dst, key, e), ranks from the
    row starts."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    nnz = src.shape[0]
    keep = np.zeros(nnz, dtype=bool)
    loop = (src == dst) if keep_loops else np.zeros(nnz, dtype=bool)
    keep[loop] = True
    cand = np.flatnonzero(~loop)
    if cand.size:
        k = keys(seed, offset, nnz)[cand]
        d = dst[cand]
        o = np.lexsort((cand, k, d))  # last key first: dst, then key, then COO id
        ds = d[o]
        start = np.flatnonzero(np.r_[True, ds[1:] != ds[:-1]])
        seg = np.cumsum(np.r_[True, ds[1:] != ds[:-1]]) - 1
        rank = np.arange(cand.size) - start[seg]
        keep[cand[o]] = rank < fanout
    if rows is not None:
        keep &= np.asarray(rows, dtype=bool)[dst]
    return keep
