"""numpy restatement of the decoder's dropout mask (lavila_amd/csrc/dropout.h), written from the specification and not from
the kernel source: Philox4x32-10 with the standard constants, counter = (element group, site), key = seed.

    g   = e >> 2
    ctr = (g & 0xffffffff, g >> 32, site, 0)
    key = (seed & 0xffffffff, seed >> 32)
    w   = philox4x32_10(ctr, key)[e & 3]
    T   = min(2^32 - 1, floor(p * 2^32 + 0.5))       p a float32
    keep iff w >= T;  scale = float32(1) / (float32(1) - p)

Row sites over [rows, D] use e = row * D + col; attention sites e = (((b * H + h) * L + i) << 8) | j (query i, key j < 256).
Sites: 0 the embedding, block i 1 + 6 i + k with k = 0 cross-attention probabilities, 1 cross c_proj output,
2 mlp_crossattention output, 3 self-attention probabilities, 4 self c_proj output, 5 mlp output.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# known answers of Philox4x32-10 (Random123's kat_vectors): counter, key -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (values < 2^32) of one shape, key: two ints -> four uint64 arrays (values < 2^32)."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & m32
        h1, l1 = p1 >> np.uint64(32), p1 & m32
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def threshold(p):
    p = float(np.float32(p))
    return min(MASK32, int(np.floor(p * 4294967296.0 + 0.5)))


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(seed, site, elem0, n):
    """The random word of each of the elements elem0 .. elem0 + n - 1 (uint64 array of values < 2^32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g0, g1 = elem0 >> 2, (elem0 + n - 1) >> 2
    g = np.arange(g1 - g0 + 1, dtype=np.uint64) + np.uint64(g0)
    zero = np.zeros_like(g)
    out = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), zero + np.uint64(site), zero),
                        (seed & MASK32, seed >> 32))
    flat = np.stack(out, axis=1).reshape(-1)
    off = elem0 - (g0 << 2)
    return flat[off:off + n]


def keep_mask(seed, site, elem0, n, p):
    """bool [n]: keep of elements elem0 .. elem0 + n - 1."""
    return words(seed, site, elem0, n) >= np.uint64(threshold(p))


def row_mask(seed, site, rows, D, p):
    """bool [rows, D] of a row site (e = row * D + col)."""
    return keep_mask(seed, site, 0, rows * D, p).reshape(rows, D)


def attn_mask(seed, site, B, H, L, Tk, p):
    """bool [B, H, L, Tk] of an attention site (e = (((b * H + h) * L + i) << 8) | j)."""
    assert Tk <= 256
    return keep_mask(seed, site, 0, B * H * L * 256, p).reshape(B, H, L, 256)[..., :Tk]


def site_of(block, k):
    return 1 + 6 * block + k
