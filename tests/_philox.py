"""NumPy restatement of the sampler's latent draws (include/mra_hip.h, mra_sample): Philox4x32-10 with key = seed (lo, hi) and
counter = (slot lo, slot hi, sample lo, sample hi), then u1 = ((w0 + 2^32 w1) >> 11 + 0.5) 2^-53, u2 likewise from (w2, w3),
z = sqrt(-2 log u1) cos(2 pi u2)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: (4, n) uint32, key: (2,) or (2, n) uint32 -> (4, n) uint32."""
    c = [np.asarray(x, dtype=np.uint32).copy() for x in ctr]
    k0 = np.asarray(key[0], dtype=np.uint32).copy()
    k1 = np.asarray(key[1], dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0 = k0 + W0
            k1 = k1 + W1
    return np.array(c, dtype=np.uint32)


def latent_draws(seed, slots, samples):
    """z[s, k] for the sample numbers `samples` (global, i.e. sample0 + s) and latent slots `slots`."""
    slots = np.asarray(slots, dtype=np.uint64)
    samples = np.asarray(samples, dtype=np.uint64)
    S, K = np.meshgrid(samples, slots, indexing="ij")
    S, K = S.ravel(), K.ravel()
    ctr = [(K & MASK).astype(np.uint32), (K >> np.uint64(32)).astype(np.uint32),
           (S & MASK).astype(np.uint32), (S >> np.uint64(32)).astype(np.uint32)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)))
    a = w[0].astype(np.uint64) | (w[1].astype(np.uint64) << np.uint64(32))
    b = w[2].astype(np.uint64) | (w[3].astype(np.uint64) << np.uint64(32))
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((b >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return z.reshape(len(samples), len(slots))
