"""numpy uint64 restatement of checksum_kernel (csrc/dit_elementwise.hip): the content fingerprint that decides whether the sampler's
conditioning is step-invariant (wan_transformer3d_FlexAM.py:598-614).  For a buffer of n bytes, n_words = n // 4 little-endian 32-bit
words w_i and n % 4 tail bytes t_j:

    x_i = w_i + (i + 1) * G                     G = 0x9E3779B97F4A7C15 (golden-ratio constant), all mod 2^64
    x_t = t_j + (n_words + 1 + j) * G
    s0  = sum mix(x) + mix(n)                   over every word and tail byte; mix = the splitmix64 finaliser
    s1  = sum mix(x ^ 0xD6E8FEB86659FD93)

returned as signed 64-bit integers, the way flexam_amd.hip.checksums reads them back."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
K1 = np.uint64(0xD6E8FEB86659FD93)


def mix(x):
    """splitmix64 finaliser, elementwise on a uint64 array (wraps mod 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def checksum(data: bytes):
    """(s0, s1) of a byte string, as two signed int64 Python ints."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size
    nw = n // 4
    words = buf[:nw * 4].view("<u4").astype(np.uint64)
    tail = buf[nw * 4:].astype(np.uint64)
    x = np.concatenate([words, tail]) + np.arange(1, n - 3 * nw + 1, dtype=np.uint64) * G
    s0 = np.sum(np.concatenate([mix(x), mix(np.array([n], dtype=np.uint64))]), dtype=np.uint64)
    s1 = np.sum(mix(x ^ K1), dtype=np.uint64)
    return tuple(int(v) for v in np.array([s0, s1], dtype=np.uint64).view(np.int64))
