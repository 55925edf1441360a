"""A numpy restatement of mgcn.sample_blocks's definition, on top of
sample_ref.sample_keep: the yardstick of tests/test_block_host.py and
tests/test_gpu_blocks.py.

Frontiers grow from the seeds outwards: F_L = seeds in the order given; for
l = L-1 .. 0 the destinations D = F_{l+1} keep the parent COO edges of
sample_keep(fanouts[l], seed, offset + l, keep_loops, rows=mask(D)), ordered by
(position of dst in D, parent COO id); F_l is D followed by the sources of
those edges outside D in ascending id; a node's local id is its position in
F_l."""
import numpy as np

import sample_ref as sr


def blocks(src, dst, n, seeds, fanouts, seed, offset, keep_loops=True):
    """Per layer l = 0 .. L-1: (src_ids int64 [n_src], n_dst, edge_index int64
    [2, nnz_b] in local ids, parent_eid int64 [nnz_b])."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    D = np.asarray(seeds, dtype=np.int64).reshape(-1)
    out = [None] * len(fanouts)
    for l in range(len(fanouts) - 1, -1, -1):
        mask = np.zeros(n, dtype=bool)
        mask[D] = True
        keep = sr.sample_keep(src, dst, n, fanouts[l], seed, offset + l, keep_loops, rows=mask)
        pos = np.full(n, -1, dtype=np.int64)
        pos[D] = np.arange(D.size)
        e = np.flatnonzero(keep)
        e = e[np.lexsort((e, pos[dst[e]]))]  # last key first: position in D, then COO id
        new = np.zeros(n, dtype=bool)
        new[src[e]] = True
        new[D] = False
        src_ids = np.concatenate([D, np.flatnonzero(new)])
        local = np.full(n, -1, dtype=np.int64)
        local[src_ids] = np.arange(src_ids.size)
        out[l] = (src_ids, int(D.size), np.stack([local[src[e]], pos[dst[e]]]), e)
        D = src_ids
    return out
