"""A numpy restatement of mgcn_edge_noise's definition (include/mgcn.h): the
yardstick of tests/test_edge_noise_host.py and tests/test_gpu_edge_noise.py.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
as 1, 2, 3", SC'11), the counter layout (e, h / 4, offset lo, offset hi) under
the key (seed lo, seed hi), u = (word >> 8) * 2^-24, and the two transforms in
fp32 (numpy's fp32 operations in the reference's order) and fp64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: (k0, k1) python ints -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., j].astype(np.uint64) for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # < 2^64: both factors < 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(seed, offset, nnz, H, eid=None):
    """u as float32 [nnz, H] (exact: 24 bits); eid None: e = k."""
    e = np.arange(nnz, dtype=np.uint32) if eid is None else np.asarray(eid).astype(np.uint32)
    Q = (H + 3) // 4
    ctr = np.empty((nnz, Q, 4), dtype=np.uint32)
    ctr[:, :, 0] = e[:, None]
    ctr[:, :, 1] = np.arange(Q, dtype=np.uint32)[None, :]
    ctr[:, :, 2] = offset & 0xFFFFFFFF
    ctr[:, :, 3] = (offset >> 32) & 0xFFFFFFFF
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = words.reshape(nnz, Q * 4)[:, :H]
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def gumbel32(u):
    """-log(-log(u + 1e-20) + 1e-20), every operation in fp32."""
    u = np.asarray(u, dtype=np.float32)
    eps = np.float32(1e-20)
    a = -np.log(u + eps, dtype=np.float32)
    return -np.log(a + eps, dtype=np.float32)


def gumbel64(u):
    """The same formula in fp64 on the exact u."""
    u = np.asarray(u, dtype=np.float64)
    return -np.log(-np.log(u + 1e-20) + 1e-20)


def dropout_scale(p):
    """The kept value: one fp32 division (inf at p = 1, where nothing is kept)."""
    with np.errstate(divide="ignore"):
        return np.float32(1) / (np.float32(1) - np.float32(p))


def dropout_keep(u, p):
    return np.asarray(u, dtype=np.float32) >= np.float32(p)


def dropout32(u, p):
    keep = dropout_keep(u, p)
    out = np.zeros(keep.shape, dtype=np.float32)
    out[keep] = dropout_scale(p)
    return out
