"""The in-launch Gumbel draw of include/macm.h (macm_sample_config) in numpy, written from the
definition and not from the kernel (tests/ only): the reference that macm_policy_noise,
macm_policy_flock_sampled and the sampled rollouts are compared with.

    words   w[0..3] = Philox4x32-10(counter = (first_row + r, lo32(d), hi32(d), h), key = (lo32(seed), hi32(seed)))
            word c < 3 belongs to logit 3h + c, word 3 is unused; first_row + rows <= 2**32
    uniform u = (float64(w) + 0.5) * 2**-32          (exact)
    noise   g = float32(-log(-log(u)))               (float64 logs, one final rounding)

Philox is held in uint64 arrays (a 32 x 32 bit product fits); `philox_int` is the same generator in
Python ints, for the cross-check."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
U64 = np.uint64

# (counter, key, words): the three known answers of the standard generator
KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox_int(ctr, key):
    """Philox4x32-10 on Python ints: ctr (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 elementwise: six broadcastable arrays of 32-bit values -> uint32 [..., 4]."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, U64) & U64(MASK) for v in (c0, c1, c2, c3, k0, k1)))
    s32, m = U64(32), U64(MASK)
    for _ in range(10):
        p0, p1 = U64(M0) * c0, U64(M1) * c2  # < 2**64: exact
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + U64(W0)) & m, (k1 + U64(W1)) & m
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, decision, n_dec, rows, first_row=0):
    """uint32 [n_dec, rows, 3, 4]: the words of decisions decision .. decision + n_dec - 1, the job's rows
    first_row + r for r < rows, heads 0..2 (what macm_policy_noise_at exports)."""
    seed, decision, first_row = int(seed), int(decision), int(first_row)
    if not (0 <= first_row and first_row + rows <= 2**32):
        raise ValueError("first_row + rows must be in [0, 2**32]: the row is a 32-bit counter word")
    d = np.array([(decision + j) & (2**64 - 1) for j in range(n_dec)], dtype=U64).reshape(n_dec, 1, 1)
    r = (U64(first_row) + np.arange(rows, dtype=U64)).reshape(1, rows, 1)
    h = np.arange(3, dtype=U64).reshape(1, 1, 3)
    return philox(r, d & U64(MASK), d >> U64(32), h, U64(seed & MASK), U64(seed >> 32))


def uniform(w):
    """u = (float64(w) + 0.5) * 2**-32, exact and strictly inside (0, 1)."""
    return (np.asarray(w, np.uint32).astype(np.float64) + 0.5) * 2.0**-32


def gumbel64(w):
    """-log(-log(u)) in float64, before the final rounding."""
    return -np.log(-np.log(uniform(w)))


def noise_of_words(w):
    """float32 [..., 9] from words [..., 3, 4]: logit 3h + c takes word c of head h."""
    w = np.asarray(w, np.uint32)
    return gumbel64(w[..., :3]).astype(np.float32).reshape(w.shape[:-2] + (9,))


def noise(seed, decision, n_dec, rows, first_row=0):
    """float32 [n_dec, rows, 9]: the noise of macm_policy_noise_at (first_row = 0: macm_policy_noise)."""
    return noise_of_words(words(seed, decision, n_dec, rows, first_row))
